"""Morlet plans on every kernel and path they reach, w0 from 2 to 20.  Every case names the branch it targets, asserts
through the plan's hooks that the plan still reaches it (morlet_cases.levels / kernel: api.cpp's level_kernel for a
Morlet plan -- k_synth when synth16 = 1 on an unshifted level or when the level is unshifted and not fast (halo > 48 or
more than 256 scales), else k_synth7, its WIDE build when halo > 48), and then compares with the truth: per epoch the
float64 overlap-add convolution of the mean-removed recording with Morlet(w0, f, fs).get_wavelet() (morlet_cases.truth),
metric conftest.rel_err, gate TOL = 1e-5 (2 TOL on power rows, the square).  tests/test_morlet_model_cpu.py holds the
float64 model of the same layouts within a quarter of the gate.

  a  bank                 k_build_bank's Morlet branch, k_gain_rows_complex / k_bank_gain after a broadcast
  b  k_synth7<CG>         default grid, N = 70 001, w0 = 2 .. 20; the selection options
  c  k_synth7<WIDE, CG>   N = 1e6 at w0 = 4, 5, 5.5 (a shifted level of R = 256, halo > 100); four epochs
  d  k_synth              synth16 = 1, a level of 300 scales, unshifted halos beyond 48 (w0 = 20, support_tol = 1e-9)
  e  full band            the 18 .. 19 scales below R = 256's reach of (c)'s plans, the full-band options
  f  block convolution and time domain
  g  layouts              recordings shorter than the kernels, batches of epochs, channels, pitch, graphs
  h  time blocks          9e6 samples at 30 kHz, three segments
  i  output stride        k_synth7s<CG>
  j  steep spectra        shifted levels have no low cut: the default call's watch
"""
import math

import numpy as np
import pytest

import morlet_cases as mc
import morlet_model
from conftest import rel_err
from morlet_cases import TOL, as_output, gate, kernel, levels, truth
from test_gpu_output_stride_matrix import _Layout, _phase_ks, _ranges

pytestmark = pytest.mark.gpu

FS = 1000.0
N_GRID = 70001
OUTPUTS = ["amplitude", "power", "complex"]
_CACHE = {}


def _note(family, name, err, output="complex"):
    err = np.asarray(err)
    print("(%s) %s [%s]: worst row %.2e (gate %.0e), median %.2e" % (family, name, output, err.max(), gate(output),
                                                                     np.median(err)))


def _lfp(c, n, fs=FS, seed=11):
    from ghost_amd.synthetic import lfp
    return lfp(c, n, fs, seed=seed)


def _plan(x, f, w0, output="complex", fs=FS, **kw):
    from ghost_amd.engine import CwtPlan
    x = np.atleast_2d(x)
    return CwtPlan(x.shape[1], x.shape[0], fs, f, morlet_w0=w0, output=output, **kw)


def _grid_case(w0):
    """Two channels of LFP (one seed each), N = 70 001, the default grid of w0, the truth of both channels."""
    if w0 not in _CACHE:
        x = np.stack([_lfp(1, N_GRID, seed=11)[0], _lfp(1, N_GRID, seed=12)[0]])
        f = mc.default_grid(w0, N_GRID, FS)
        _CACHE[w0] = (x, f, np.stack([truth(x[c], FS, f, w0, threads=8) for c in range(2)]))
    return _CACHE[w0]


def _check(family, name, got, ref, output):
    err = rel_err(got, as_output(output, ref))
    _note(family, name, err, output)
    assert err.max() <= gate(output), (name, output, np.unravel_index(np.argmax(err), err.shape), err.max())


def _two_sided(lv, w0):
    if w0 < mc.TWO_SIDED_BELOW:
        assert all(l["band_shift"] > 0 and l["low_cut"] == 0 for l in lv), lv
    else:
        assert all(l["band_shift"] == 0 for l in lv), lv


# ---- a: the bank ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w0", [2.0, 5.0, 6.0, 20.0])
def test_a_bank_is_the_closed_form_and_survives_a_broadcast(w0):
    """k_build_bank's Morlet branch: row s holds H_s at bins k - band_shift of 256 R, a float64 value rounded once --
    within 1.01 sqrt(2) 2^-24 of the row's peak (the bound test_direct_kernel_is_get_wavelet derives) wherever the
    model's own truncation (three aliases against six) is below a hundredth of that.  Then gcwt_comm_broadcast_bank on
    a one-rank communicator (k_bank_gain's Morlet branch and k_gain_rows_complex a second time): the bank and a
    following execute bit-equal to before."""
    import ctypes as C
    from ghost_amd import _lib
    from ghost_amd._lib import lib, check, COMM_ID_BYTES
    x, f, _ = _grid_case(w0)
    p = _plan(x, f, w0)
    lv = levels(p)
    _two_sided(lv, w0)
    before = p.execute(x)
    bank = p.filter_bank()
    bound = 1.01 * np.sqrt(2.0) * 2.0 ** -24
    k, worst, compared = np.arange(256), 0.0, 0
    for l in lv:
        theta = 2 * np.pi * (k - l["band_shift"]) / (256.0 * l["decimation"])
        for s in l["scales"]:
            ref = morlet_model.response(theta, w0, f[s], FS, aliases=6)
            peak = np.abs(ref).max()
            ok = np.abs(morlet_model.response(theta, w0, f[s], FS, aliases=3) - ref) <= 0.01 * bound * peak
            assert ok.sum() >= 250, (w0, s, ok.sum())
            err = np.abs(bank[s] - ref)[ok].max() / peak
            worst, compared = max(worst, err), compared + 1
            assert err <= bound, (w0, l["decimation"], s, err)
    assert compared == (p.scale_info()["method"] == _lib.SCALE_SPECTRAL).sum() >= 60
    print("(a) w0=%g: %d bank rows, worst %.2e of the peak (bound %.2e)" % (w0, compared, worst, bound))
    ident = C.create_string_buffer(COMM_ID_BYTES)
    check(lib.gcwt_comm_unique_id(ident))
    comm = C.c_void_p()
    check(lib.gcwt_comm_create(C.byref(comm), 0, 1, ident))
    check(lib.gcwt_comm_broadcast_bank(comm, p._handle, 0))
    np.testing.assert_array_equal(p.filter_bank(), bank)
    np.testing.assert_array_equal(p.execute(x), before)
    lib.gcwt_comm_destroy(comm)
    p.close()


# ---- b: k_synth7<CG> ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w0", mc.W0S)
def test_b_default_grid_every_row(w0):
    """k_synth7's complex-gain build on every level (halo <= 48 everywhere at this length), shifted below w0 = 5.6;
    w0 = 20: halos next to the 48 limit; w0 <= 4: seven or more time-domain scales (morlet_tap); w0 >= 10: block
    convolution at the top of the grid.  Every row, all three outputs, both channels."""
    from ghost_amd import _lib
    x, f, ref = _grid_case(w0)
    for output in OUTPUTS:
        p = _plan(x, f, w0, output)
        lv, si = levels(p), p.scale_info()
        assert p.info["n_interp"] == 0 and len(lv) >= 7 and all(kernel(l) == "k_synth7" for l in lv), lv
        _two_sided(lv, w0)
        if w0 == 20.0:
            assert sum(l["halo"] >= 40 for l in lv) >= 5
        if w0 <= 4.0:
            assert (si["method"] == _lib.SCALE_DIRECT).sum() >= 7 and si["length"].min() <= 31
        if w0 >= 10.0:
            assert len(p.debug_blockconv()) >= 1 and (si["method"] == _lib.SCALE_BLOCKCONV).sum() >= 3
        _check("b", "w0=%g default grid, %d rows" % (w0, f.size), p.execute(x), ref, output)
        p.close()


B_OPTIONS = [("synth_cols", 16, False), ("synth7_narrow_r", 0, False), ("synth7_narrow_r", 2, False),
             ("synth7_narrow_r", 4, False), ("fuse_blocks", 0, False), ("synth7_order", 1, True),
             ("synth7_order", 2, True), ("level_streams", 0, True), ("synth_streams", 1, True)]


@pytest.mark.parametrize("w0", [5.0, 6.0])
def test_b_selection_options(option, w0):
    """Every selection option that touches k_synth7 on a Morlet plan, each against the truth (complex and amplitude).
    The Morse tests of these options (test_synthesis_kernels_agree, test_split_levels_option) ask for agreement to
    rounding, not bit equality; the options that only reorder or reschedule the same work items (synth7_order,
    level_streams, synth_streams) are held bit-equal to the default plan here."""
    x, f, ref = _grid_case(w0)
    base = {}
    for output in ("complex", "amplitude"):
        p = _plan(x, f, w0, output)
        base[output] = p.execute(x)
        p.close()
    for name, value, same in B_OPTIONS:
        option(name, value)
        for output in ("complex", "amplitude"):
            p = _plan(x, f, w0, output)
            assert all(kernel(l) == "k_synth7" for l in levels(p)) and p.info["n_interp"] == 0
            got = p.execute(x)
            p.close()
            _check("b", "w0=%g %s=%d" % (w0, name, value), got, ref, output)
            if same:
                np.testing.assert_array_equal(got, base[output], err_msg="%s=%d" % (name, value))
        option(name, None)


# ---- c, e: the wide halo on a shifted band; full band -----------------------------------------------------------------

def _fetch(res, rows):
    return np.stack([res.to_host(scales=slice(r, r + 1))[0, 0] for r in rows])


def _million(w0):
    key = ("1e6", w0)
    if key not in _CACHE:
        from ghost_amd import _lib
        n = 1000000
        x = _lfp(1, n, seed=5)
        f = mc.default_grid(w0, n, FS)
        p = _plan(x, f, w0, "amplitude")
        wide = [l for l in levels(p) if kernel(l) == "k_synth7w"]
        assert len(wide) == 1 and wide[0]["decimation"] == 256 and wide[0]["scales"].size >= 5, levels(p)
        halo = wide[0]["halo"]
        rows = mc.row_subset(p, np.random.default_rng(16), extra=2,
                             whole=lambda key: key[0] == _lib.SCALE_FULLBAND or key[2] == halo)
        p.close()
        _CACHE[key] = (x, f, rows, truth(x[0], FS, f, w0, rows=rows, threads=8))
    return _CACHE[key]


@pytest.mark.parametrize("w0", [4.0, 5.0, 5.5])
def test_c_e_wide_halo_level_and_full_band_at_1e6(w0):
    """N = 1e6, default grid: a shifted level of R = 256 whose halo is beyond 48 -> k_synth7<WIDE, CG> (items7w), every
    row of it; and, since a two-sided band cannot go above R = 256, 15 or more full-band scales with kernels of well
    over 100 000 taps (k_fullband_filter's closed form with the delay), every one; one row of every other
    (method, decimation, halo) group.  Amplitude and complex."""
    from ghost_amd import _lib
    x, f, rows, ref = _million(w0)
    for output in ("amplitude", "complex"):
        p = _plan(x, f, w0, output)
        lv, si = levels(p), p.scale_info()
        wide = [l for l in lv if kernel(l) == "k_synth7w"]
        assert len(wide) == 1 and wide[0]["band_shift"] > 0 and wide[0]["halo"] > 48 and wide[0]["scales"].size >= 5
        full = np.flatnonzero(si["method"] == _lib.SCALE_FULLBAND)
        assert full.size >= 15 and si["length"][full].max() > 150000 and p.info["n_interp"] == 0
        assert set(wide[0]["scales"].tolist()) | set(full.tolist()) <= set(rows)
        res = p.execute_resident(x)
        got = _fetch(res, rows)
        res.free()
        p.close()
        err = rel_err(got, as_output(output, ref))
        is_full, is_wide = np.isin(rows, full), np.isin(rows, wide[0]["scales"])
        _note("c", "w0=%g 1e6 wide level (halo %d, %d rows)" % (w0, wide[0]["halo"], is_wide.sum()), err[is_wide], output)
        _note("e", "w0=%g 1e6 full band (%d rows, up to %d taps)" % (w0, is_full.sum(), si["length"][full].max()),
              err[is_full], output)
        _note("c", "w0=%g 1e6 other groups" % w0, err[~is_full & ~is_wide], output)
        assert err.max() <= gate(output), (w0, output, rows[int(np.argmax(err))], err.max())


def test_c_four_epochs():
    """Four epochs (two touching, a 700-sample one, two gaps) at w0 = 5: a wide-halo level at R = 64 beside the fast one,
    every segment with its own lead; gaps exactly 0.  All three outputs, every row."""
    x = _lfp(1, mc.FOUR_EPOCHS_N, seed=3)
    ref = truth(x[0], FS, mc.FOUR_EPOCHS_F, 5.0, bounds=mc.FOUR_EPOCHS, threads=8)
    outside = np.ones(mc.FOUR_EPOCHS_N, bool)
    for a, b in mc.FOUR_EPOCHS:
        outside[a:b] = False
    for output in OUTPUTS:
        p = _plan(x, mc.FOUR_EPOCHS_F, 5.0, output, epoch_bounds=mc.FOUR_EPOCHS)
        lv = levels(p)
        assert any(kernel(l) == "k_synth7w" and l["band_shift"] > 0 and l["scales"].size >= 3 for l in lv), lv
        assert any(kernel(l) == "k_synth7" for l in lv) and len(p.segments()) == 4
        got = p.execute(x)[0]
        p.close()
        assert outside.any() and not got[:, outside].any()
        _check("c", "four epochs w0=5", got, ref, output)


E_OPTIONS = [("fullband4", 0), ("fullband4", 1), ("fullband_group", 4), ("fullband_group", 16), ("fullband_cache_mb", 0)]


def test_e_full_band_options(option):
    """The full-band options on (c)'s w0 = 5 plan: sets of four or single scales, two group sizes of the fused row pass,
    no response cache.  Every full-band row against the truth; the rows of all variants bit-equal among themselves
    (the options regroup the same arithmetic)."""
    from ghost_amd import _lib
    x, f, rows, ref = _million(5.0)
    first = None
    for name, value in E_OPTIONS:
        option(name, value)
        p = _plan(x, f, 5.0, "complex")
        full = np.flatnonzero(p.scale_info()["method"] == _lib.SCALE_FULLBAND)
        assert full.size >= 15 and set(full.tolist()) <= set(rows)
        res = p.execute_resident(x)
        got = _fetch(res, full)
        res.free()
        p.close()
        option(name, None)
        _check("e", "w0=5 1e6 %s=%d" % (name, value), got, ref[np.isin(rows, full)], "complex")
        if first is None:
            first = got
        np.testing.assert_array_equal(got, first, err_msg="%s=%d" % (name, value))


# ---- d: k_synth reading a Morlet bank -----------------------------------------------------------------------------

@pytest.mark.parametrize("w0", [6.0, 10.0])
def test_d_synth16_moves_every_unshifted_level(option, w0):
    x, f, ref = _grid_case(w0)
    option("synth16", 1)
    for output in OUTPUTS:
        p = _plan(x, f, w0, output)
        lv = levels(p)
        assert len(lv) >= 7 and all(kernel(l, synth16=True) == "k_synth" and l["band_shift"] == 0 for l in lv), lv
        _check("d", "w0=%g synth16=1" % w0, p.execute(x), ref, output)
        p.close()


def test_d_synth16_leaves_shifted_levels_on_k_synth7(option):
    """w0 = 5: every level is shifted, so synth16 = 1 moves none (the 16-column kernel knows no band shift).  The option
    still takes the block transforms out of k_synth7 (api.cpp: fused_blocks needs synth16 off), so the rows are those
    of the fuse_blocks = 0 plan, bit for bit -- not the default plan's, whose block spectra k_synth7 makes itself and
    rounds differently -- and within the gate."""
    x, f, ref = _grid_case(5.0)
    for output in ("complex", "amplitude"):
        option("fuse_blocks", 0)
        p = _plan(x, f, 5.0, output)
        want = p.execute(x)
        p.close()
        option("fuse_blocks", None)
        option("synth16", 1)
        p = _plan(x, f, 5.0, output)
        assert all(l["band_shift"] > 0 and kernel(l, synth16=True) == "k_synth7" for l in levels(p))
        got = p.execute(x)
        p.close()
        option("synth16", None)
        np.testing.assert_array_equal(got, want)
        _check("d", "w0=5 synth16=1 (no level moves)", got, ref, output)


def test_d_level_of_300_scales_and_unshifted_wide_halos():
    """k_synth as the fallback: one unshifted level of 300 scales (more than k_synth7's 256), every fifth row and the two
    ends; and w0 = 20 with support_tol = 1e-9, whose unshifted levels need halos beyond 48, every row."""
    x = _lfp(1, N_GRID, seed=13)
    f = np.geomspace(60.0, 40.0, 300)
    rows = sorted(set(range(0, 300, 5)) | {299})
    ref = truth(x[0], FS, f, 6.0, rows=rows, threads=8)
    for output in ("complex", "power"):
        p = _plan(x, f, 6.0, output)
        lv = levels(p)
        assert len(lv) == 1 and lv[0]["scales"].size == 300 and kernel(lv[0]) == "k_synth", lv
        _check("d", "300 scales on one level", p.execute(x)[0][rows], ref, output)
        p.close()
    x, f, ref = _grid_case(20.0)
    for output in ("complex", "amplitude"):
        p = _plan(x, f, 20.0, output, support_tol=1e-9)
        lv = levels(p)
        slow = [l for l in lv if l["halo"] > 48 and l["band_shift"] == 0 and kernel(l) == "k_synth"]
        assert len(slow) >= 5 and sum(l["scales"].size for l in slow) >= 50, lv
        _check("d", "w0=20 support_tol=1e-9 (halos %d .. %d)" % (min(l["halo"] for l in slow), max(l["halo"] for l in slow)),
               p.execute(x), ref, output)
        p.close()


# ---- f: block convolution and the time domain ------------------------------------------------------------------------

def test_f_block_convolution_and_exact_paths(option):
    """direct_max_len = 0 at w0 = 6 (the top of the grid by block convolution instead of the time domain);
    blockconv = 0 with direct_max_len = 128 at w0 = 10 (its shortest kernels, 59 taps and up, in the time domain);
    precision = 'exact' at w0 = 6 (no decimated path: block convolution and full band only).  (w0 = 10 and 20 with
    their default block-convolution scales are in test_b_default_grid_every_row.)"""
    from ghost_amd import _lib
    x, f, ref = _grid_case(6.0)
    option("direct_max_len", 0)
    p = _plan(x, f, 6.0)
    m = p.scale_info()["method"]
    assert (m == _lib.SCALE_DIRECT).sum() == 0 and (m == _lib.SCALE_BLOCKCONV).sum() >= 4 and p.debug_blockconv()
    _check("f", "w0=6 direct_max_len=0", p.execute(x), ref, "complex")
    p.close()
    option("direct_max_len", None)
    for output in ("complex", "amplitude"):
        p = _plan(x, f, 6.0, output, precision="exact")
        m = p.scale_info()["method"]
        assert (m == _lib.SCALE_BLOCKCONV).sum() >= 30 and (m == _lib.SCALE_FULLBAND).sum() >= 30 and not levels(p)
        assert (m == _lib.SCALE_SPECTRAL).sum() == 0 and len(p.debug_blockconv()) >= 2
        _check("f", "w0=6 precision='exact'", p.execute(x), ref, output)
        p.close()
    x, f, ref = _grid_case(10.0)
    option("blockconv", 0)
    option("direct_max_len", 128)
    p = _plan(x, f, 10.0)
    si = p.scale_info()
    direct = si["method"] == _lib.SCALE_DIRECT
    assert direct.sum() >= 3 and (si["method"] == _lib.SCALE_BLOCKCONV).sum() == 0 and si["length"][direct].max() >= 64
    _check("f", "w0=10 blockconv=0 direct_max_len=128", p.execute(x), ref, "complex")
    p.close()


def test_f_time_domain_kernel_every_alignment_and_edge(option):
    """The cases of test_gpu_parity.test_time_domain_kernel_every_alignment_and_edge with Morlet taps (morlet_tap,
    w0 = 2: the default grid's own time-domain kernels start at 21 taps): one frequency per kernel length 21 .. 52, so
    every residue of (L - 1) // 2 mod 8 and both parities of the group count (longer Morlet kernels are band-limited
    and planned spectral whatever direct_max_len says: four of them ride along); three channels with offsets, two
    epochs two samples apart, all outputs, tiles that end inside the range and block requests whose first column is
    no multiple of four."""
    from ghost_amd import _lib
    from ghost_amd.wave import Morlet
    w0 = 2.0
    option("direct_max_len", 256)
    n = 6200
    rng = np.random.default_rng(77)
    x = (rng.standard_normal((3, n)) + np.array([[0.7], [-2.0], [0.0]])).astype(np.float32)
    grid = np.geomspace(270.0, 20.0, 6001)
    lens = Morlet(w0=w0, fs=FS).compute_lengths(grid / (FS / 2.0) * np.pi)
    f = np.array([grid[lens == L].max() for L in list(range(21, 53)) + [97, 160, 231, 250] if np.any(lens == L)])
    assert f.size == 36
    eb = np.array([[0, 2501], [2503, n]])
    ref = np.stack([truth(x[c], FS, f, w0, bounds=eb) for c in range(3)])
    for output in ("complex", "amplitude", "power"):
        p = _plan(x, f, w0, output, epoch_bounds=eb)
        si = p.scale_info()
        direct = si["method"] == _lib.SCALE_DIRECT
        assert direct.sum() >= 32 and si["length"][direct].min() == 21 and si["length"][direct].max() >= 52, si["method"]
        assert len({int((L - 1) // 2) % 8 for L in si["length"][direct]}) == 8
        assert len({int(-(-L // 8)) % 2 for L in si["length"][direct]}) == 2
        got = p.execute(x)
        _check("f", "time domain, w0=2 taps of %d .. %d" % (si["length"][direct].min(), si["length"][direct].max()),
               got[:, direct], ref[:, direct], output)
        _check("f", "their spectral neighbours", got[:, ~direct], ref[:, ~direct], output)
        assert np.all(got[:, :, 2501:2503] == 0)
        for start, length in [(1, 2047), (2049, 2050), (2502, 3698), (3, 1)]:
            np.testing.assert_array_equal(p.execute_block(x, start, length), got[:, :, start:start + length])
        p.close()


# ---- g: layouts -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 5, 37, 64, 255, 1000])
def test_g_recordings_shorter_than_the_kernels(n):
    """Kernels of 74 .. 292 taps on recordings of 1 .. 1000 samples: planned spectral (k_synth7<CG> on blocks that are
    mostly padding).  Three channels, all outputs."""
    from ghost_amd import _lib
    f = np.array([200.0, 100.0, 50.0])
    rng = np.random.default_rng(n)
    x = (rng.standard_normal((3, n)) + np.array([[0.0], [1.5], [-30.0]])).astype(np.float32)
    ref = np.stack([truth(x[c], FS, f, 6.0) for c in range(3)])
    for output in OUTPUTS:
        p = _plan(x, f, 6.0, output)
        si = p.scale_info()
        assert (si["method"] == _lib.SCALE_SPECTRAL).all() and si["length"].min() == 74 and si["length"].max() == 292
        assert all(kernel(l) == "k_synth7" for l in levels(p))
        got = p.execute(x)
        p.close()
        if n == 1:                      # one sample less its own mean: the truth is 0, and so must the result be
            assert not ref.any() and not got.any()
            continue
        _check("g", "N=%d" % n, got, ref, output)


def _many_epochs():
    """20 epochs of 4000 samples in a row, then 20 of ragged lengths (900 .. 6000) with gaps of 0 .. 300 samples."""
    rng = np.random.default_rng(2020)
    eb, pos = [[4000 * i, 4000 * (i + 1)] for i in range(20)], 80000
    for i in range(20):
        pos += int(rng.integers(0, 301)) if i % 4 else 0
        length = int(rng.integers(900, 6001))
        eb.append([pos, pos + length])
        pos += length
    return np.array(eb), pos + 17


def test_g_many_epochs_in_batches():
    """Segments batch by equal FFT length, 16 at most (kSegBatch): a full batch, a partial one and single-segment
    batches in one plan; three channels; gaps exactly 0; amplitude and complex, w0 = 5 (shifted) and 6."""
    eb, n = _many_epochs()
    x = _lfp(3, n, seed=20) + np.array([[0.0], [0.4], [-1.1]], np.float32)
    f = np.array([320.0, 140.0, 61.0, 33.0, 15.0])
    outside = np.ones(n, bool)
    for a, b in eb:
        outside[a:b] = False
    assert outside.sum() > 100
    for w0 in (5.0, 6.0):
        ref = np.stack([truth(x[c], FS, f, w0, bounds=eb) for c in range(3)])
        for output in ("amplitude", "complex"):
            p = _plan(x, f, w0, output, epoch_bounds=eb)
            counts = [c for _, c in p.debug_batches()]
            assert 16 in counts and 1 in counts and any(1 < c < 16 for c in counts), counts
            assert sum(counts) == len(p.segments()) == 40
            _two_sided(levels(p), w0)
            got = p.execute(x)
            assert not got[:, :, outside].any()
            _check("g", "40 epochs, batches %s, w0=%g" % (counts, w0), got, ref, output)
            np.testing.assert_array_equal(p.execute(x), got)                       # two executes bit-identical
            p.close()


def test_g_public_call_float64_input_with_an_offset():
    """float64 samples around 1e4 through transform(): the mean leaves in float64 before anything is rounded to float32."""
    from ghost_amd.wave import ContinuousWaveletTransform, Morlet
    n = 50000
    x = _lfp(1, n, seed=6)[0].astype(np.float64) + 1e4
    for w0 in (4.0, 6.0):
        cwt = ContinuousWaveletTransform(wavelet=Morlet(w0=w0))
        cwt.transform(x, fs=FS, output="complex")
        f = cwt.frequencies
        np.testing.assert_allclose(f, mc.default_grid(w0, n, FS), rtol=1e-13)
        _two_sided(levels(cwt._plan), w0)
        _check("g", "float64 + 1e4, w0=%g" % w0, cwt.coefficients, truth(x, FS, f, w0, threads=8), "complex")


def test_g_row_pitch_and_graph_replay(option):
    """Device-resident executes of a small Morlet plan: a row pitch beyond the row length; the second execute captured
    into a graph and later ones replayed (debug_graph_state() == 1), bit-equal to the eager plan and within the gate;
    w0 = 5 (shifted bands, time-domain scales) and 6."""
    from ghost_amd.engine import DeviceBuffer
    n, C = 16384, 2
    eb = np.array([[0, 9000], [9003, n]])
    xs = [_lfp(C, n, seed=s) for s in (1, 2, 3)]
    for w0 in (5.0, 6.0):
        f = mc.default_grid(w0, 7000, FS)[::3]
        option("graphs", 0)
        p0 = _plan(xs[0], f, w0, "amplitude", epoch_bounds=eb)
        eager = [p0.execute(x) for x in xs]
        option("graphs", None)
        p = _plan(xs[0], f, w0, "amplitude", epoch_bounds=eb)
        assert levels(p) and p.info["n_interp"] == 0
        _two_sided(levels(p), w0)
        xb, ob = DeviceBuffer(4 * C * n), DeviceBuffer(p.info["out_bytes"])
        for _ in range(2):
            for x, want in zip(xs, eager):              # execute 1 eager, 2 captured, 3 .. 6 replayed
                xb.upload(x)
                p.execute_device(xb, ob)
                np.testing.assert_array_equal(ob.download((C, f.size, n), np.float32), want)
        assert p.debug_graph_state() == 1 and p0.debug_graph_state() == 0
        ref = np.stack([truth(xs[2][c], FS, f, w0, bounds=eb) for c in range(C)])
        _check("g", "graph replay w0=%g" % w0, eager[2], ref, "amplitude")
        pitch = n + 96
        pb = DeviceBuffer(4 * C * f.size * pitch)
        pb.zero()
        p0.set_row_pitch(pitch)
        p0.execute_device(xb, pb)
        p0.set_row_pitch(0)
        rows = pb.download((C, f.size, pitch), np.float32)
        np.testing.assert_array_equal(rows[..., :n], eager[2])
        assert not rows[..., n:].any()
        xb.free(); ob.free(); pb.free()
        p.close(); p0.close()


# ---- h: time blocks ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w0", [6.0, 5.0])
def test_h_time_blocks_at_30_khz(w0):
    """9e6 samples at 30 kHz, 40 scales 300 .. 2 Hz, one channel, amplitude: three time blocks (segments()).  w0 = 6:
    levels up to R = 4096; w0 = 5: shifted levels up to R = 256 (one of them wide) and full-band scales with kernels of
    over 200 000 taps, in time blocks.  Truth on windows of 3000 samples at both ends and across each seam, for a
    seeded subset of rows with one of every (method, decimation, halo) group; execute_block over seeded ranges
    bit-equal to the columns of execute."""
    from ghost_amd import _lib
    from ghost_amd.synthetic import lfp_channel
    fs, n = 30000.0, 9000000
    f = np.geomspace(300.0, 2.0, 40)
    x = lfp_channel(n, fs, channel=5)[None]
    p = _plan(x, f, w0, "amplitude", fs=fs)
    segs, lv, si = p.segments(), levels(p), p.scale_info()
    assert len(segs) == 3 and p.info["n_interp"] == 0
    _two_sided(lv, w0)
    if w0 == 5.0:
        assert any(kernel(l) == "k_synth7w" for l in lv) and (si["method"] == _lib.SCALE_FULLBAND).sum() >= 5
    else:
        assert max(l["decimation"] for l in lv) >= 1024 and all(kernel(l) == "k_synth7" for l in lv)
    rows = mc.row_subset(p, np.random.default_rng(30), extra=2)
    res = p.execute_resident(x)
    mean = x[0].astype(np.float64).mean()
    w = 3000
    worst = 0.0
    # the denominator of the metric is the row's peak: the whole truth row is not made here, so the peak is read off
    # the device's row and must bound the truth on every window (a wrong scale shows in the numerator)
    peak = {r: float(res.to_host(scales=slice(r, r + 1)).max()) for r in rows}
    for a in [0, n - w] + [s[1] - w // 2 for s in segs[:-1]]:
        got = res.to_host(start=a, stop=a + w)[0]
        for r in rows:
            ref = np.abs(mc.truth_window(x[0], mean, fs, f[r], w0, a, a + w))
            assert ref.max() <= peak[r] * (1 + TOL)
            err = np.abs(got[r] - ref).max() / peak[r]
            worst = max(worst, err)
            assert err <= TOL, (w0, a, r, si["method"][r], si["decimation"][r], err)
    _note("h", "9e6 at 30 kHz w0=%g, %d rows on 4 windows" % (w0, len(rows)), np.array([worst]), "amplitude")
    rng = np.random.default_rng(9)
    ranges = [(int(rng.integers(0, n - 70000)), int(rng.integers(1, 70000))) for _ in range(3)]
    ranges += [(segs[0][1] - 4001, 9001), (segs[1][1] - 3, 5), (n - 5003, 5003)]
    for start, length in ranges:
        blk = p.execute_block(x, start, length)
        np.testing.assert_array_equal(blk, res.to_host(start=start, stop=start + length), err_msg=str((start, length)))
    res.free()
    p.close()


# ---- i: output stride with complex gains ---------------------------------------------------------------------------------

PHASE_F = np.geomspace(300.0, 0.9, 48)


def _strided_truth(family, lay, k, w0, output, b):
    key = (w0, lay.n, lay.f.tobytes(), lay.bounds.tobytes(), lay.x[:, :64].tobytes())
    if key not in _CACHE:
        _CACHE[key] = np.stack([truth(lay.x[c], lay.fs, lay.f, w0, bounds=lay.bounds, threads=8)
                                for c in range(lay.x.shape[0])])
    ref = _CACHE[key]
    want = as_output(output, ref)
    err = np.abs(b - want[..., ::k]).max(axis=-1) / np.abs(want).max(axis=-1)
    _note(family, "K=%d w0=%g" % (k, w0), err, output)
    assert err.max() <= gate(output), (k, w0, output, err.max())


@pytest.mark.parametrize("output", OUTPUTS)
@pytest.mark.parametrize("w0", [6.0, 5.0])
def test_i_phase_selection(w0, output):
    """k_synth7s<CG> on every level, R = 2 .. 256 (w0 = 6 unshifted; w0 = 5 shifted: a two-sided band stops at R = 256),
    K such that g = gcd(R, K) takes every power of two from 1 to 256: the contract of test_gpu_output_stride_matrix
    against the same plan at K = 1, and the kept columns against the truth at one K."""
    lay = _Layout(_lfp(2, N_GRID, seed=11), FS, PHASE_F, morlet_w0=w0, output=output)
    rs = sorted(l["decimation"] for l in lay.levels)
    assert all(kernel(l) == "k_synth7" and l["factor"] == 0 for l in lay.levels), lay.levels
    assert all((l["band_shift"] > 0) == (w0 == 5.0) for l in lay.levels)
    assert {2, 4, 8, 16, 32, 64, 128, 256} <= set(rs), rs
    seen = set()
    for k in _phase_ks(N_GRID):
        seen |= {math.gcd(r, k) for r in rs}
        b = lay.check(k)
        if k == 48:
            _strided_truth("i", lay, k, w0, output, b)
    assert {1, 2, 4, 8, 16, 32, 64, 128, 256} <= seen, seen
    lay.close()


@pytest.mark.parametrize("w0", [6.0, 5.0])
def test_i_segment_residues_and_narrow_levels(option, w0):
    """Three epochs of one batch whose segments start at 64, 128 and 192 mod 256, levels up to R = 256: the phase test
    of k_synth7s sees those residues (K = 128, 256, 384, 512); execute_block across epochs and gaps.  Then
    synth7_narrow_r in {0, 4}: the 16-column list beside the 32-column one."""
    n = 150000
    starts = [256 * 2 + 64 + 3, 256 * 200 + 128 + 5, 256 * 400 + 192 + 7]
    eb = np.array([[s, s + 45000] for s in starts])
    x = _lfp(2, n, seed=21) + np.array([[0.3], [-2.0]], np.float32)
    rng = np.random.default_rng(64)
    f = np.geomspace(60.0, 0.6, 12)
    for output in OUTPUTS:
        lay = _Layout(x, FS, f, morlet_w0=w0, epoch_bounds=eb, output=output)
        assert lay.full.debug_batches() == [(0, 3)]
        big = [l["decimation"] for l in lay.levels if l["decimation"] >= 256 and kernel(l) == "k_synth7"]
        assert big, lay.levels
        for k in (128, 256, 384, 512):
            b = lay.check(k, ranges=_ranges(rng, n, k, eb) if output == "amplitude" else ())
            if k == 128 and output != "power":
                _strided_truth("i", lay, k, w0, output, b)
        lay.close()
    for narrow_r in (0, 4):
        option("synth7_narrow_r", narrow_r)
        lay = _Layout(_lfp(2, 30001, seed=5), FS, PHASE_F[:20], morlet_w0=w0, output="amplitude")
        assert {2, 4, 8} <= {l["decimation"] for l in lay.levels} and all(kernel(l) == "k_synth7" for l in lay.levels)
        for k in (2, 3, 4, 6, 8, 12, 40):
            lay.check(k)
        lay.close()
        option("synth7_narrow_r", None)


def test_i_wide_halo_on_a_shifted_band():
    """(c)'s wide-halo level under a stride: N = 300 000, w0 = 5, the 27 scales of the two R = 256 levels of the default
    grid and three from further up -- the level of halo > 48 stays (k_synth7s on items7w).  K in {3, 4, 256, 1000}."""
    n, w0 = 300000, 5.0
    grid = mc.default_grid(w0, n, FS)
    from ghost_amd.engine import CwtPlan
    p = CwtPlan(n, 1, FS, grid, morlet_w0=w0)
    r256 = np.concatenate([l["scales"] for l in levels(p) if l["decimation"] == 256])
    p.close()
    f = grid[np.r_[0, 20, 40, r256]]
    x = _lfp(1, n, seed=7)
    for output in OUTPUTS:
        lay = _Layout(x, FS, f, morlet_w0=w0, output=output)
        wide = [l for l in lay.levels if kernel(l) == "k_synth7w" and l["band_shift"] > 0]
        assert wide and wide[0]["scales"].size >= 5 and wide[0]["decimation"] == 256, lay.levels
        for k in (3, 4, 256, 1000):
            b = lay.check(k)
            if k == 4 and output == "amplitude":
                _strided_truth("i", lay, k, w0, output, b)
        lay.close()


def test_i_full_band_block_convolution_and_direct_rows(option):
    """The strided stores of the other paths on Morlet plans: the top of the w0 = 10 grid (block convolution; with
    direct_max_len = 128 the time domain) and precision = 'exact' at w0 = 5 (block convolution and full band only):
    bit-equal to the K = 1 rows (the contract), and against the truth."""
    from ghost_amd import _lib
    rng = np.random.default_rng(5)
    n = 30001
    x = _lfp(2, n, seed=12)
    for direct_max_len, w0, kw, want in [(0, 10.0, {}, _lib.SCALE_BLOCKCONV), (128, 10.0, {}, _lib.SCALE_DIRECT),
                                         (None, 5.0, dict(precision="exact"), _lib.SCALE_FULLBAND)]:
        option("direct_max_len", direct_max_len)
        f = mc.default_grid(w0, n, FS)[::4] if kw else mc.default_grid(w0, n, FS)[:12]
        for output in ("amplitude", "complex"):
            lay = _Layout(x, FS, f, morlet_w0=w0, output=output, **kw)
            m = lay.full.scale_info()["method"]
            assert (m == want).any(), (w0, m)
            if kw:
                assert not (m == _lib.SCALE_SPECTRAL).any() and (m == _lib.SCALE_BLOCKCONV).any()
            for k in (2, 3, 16, 100):
                b = lay.check(k, ranges=_ranges(rng, n, k, lay.bounds, 2))
                if k == 3:
                    _strided_truth("i", lay, k, w0, output, b)
            lay.close()
    option("direct_max_len", None)


# ---- j: steep spectra --------------------------------------------------------------------------------------------------

def _steep(name, n):
    from ghost_amd.synthetic import power_law_noise, spectrum_class
    if name.endswith("_offset"):                 # as test_gpu_precision._offset builds them; the offset here 1000
        expo = {"f3_offset": 3.0, "brown_offset": 2.0}[name]
        return (power_law_noise(n, expo, 91) + 1000.0).astype(np.float32)
    return spectrum_class(name, n, FS)


@pytest.mark.parametrize("w0", [5.0, 6.0, 10.0])
@pytest.mark.parametrize("name", ["brown", "f3", "line30", "line100", "drift1000", "f3_offset", "brown_offset"])
def test_j_default_call_on_steep_spectra(name, w0):
    """Shifted Morlet levels (w0 = 5) get no low cut before the float32 stages: only the default call's watch stands
    between a steep spectrum and the gate.  N = 120 000, default grid, complex, default precision: every row."""
    from ghost_amd.wave import ContinuousWaveletTransform, Morlet
    n = 120000
    x = _steep(name, n)
    cwt = ContinuousWaveletTransform(wavelet=Morlet(w0=w0))
    cwt.transform(x, fs=FS, output="complex")
    f = cwt.frequencies
    lv = levels(cwt._plan)
    _two_sided(lv, w0)
    rep = cwt.precision_report
    assert rep["watched"]
    err = rel_err(cwt.coefficients, truth(x, FS, f, w0, threads=8))
    si = cwt._plan.scale_info()
    r = int(np.argmax(err))
    _note("j", "%s w0=%g (rerouted %d of %d, predicted worst %.2e; worst row %d: method %d R %d)" % (
        name, w0, rep["rerouted"], f.size, rep["worst"], r, si["method"][r], si["decimation"][r]), err)
    assert err.max() <= TOL, (name, w0, r, err.max())


@pytest.mark.parametrize("w0", [2.0, 4.0, 5.0, 6.0, 10.0])
def test_j_benign_recording_reroutes_nothing(w0):
    """Pink LFP stays on the fast path untouched, shifted levels included.  (The watch used to take one minimum of a
    scale's gain over both copies of a band on a shifted level, the one below zero frequency included, where a Morlet
    scale has next to none: scales below the shift frequency predicted up to 4.6e-4 where they lose 6.6e-7, and
    2 of 95 (w0 = 5), 55 of 97 (w0 = 4), 22 of 103 (w0 = 2) scales of this recording were made again for nothing.)"""
    from ghost_amd.synthetic import spectrum_class
    from ghost_amd.wave import ContinuousWaveletTransform, Morlet
    n = 120000
    x = spectrum_class("pink_lfp", n, FS)
    cwt = ContinuousWaveletTransform(wavelet=Morlet(w0=w0))
    cwt.transform(x, fs=FS, output="complex")
    _two_sided(levels(cwt._plan), w0)
    rep = cwt.precision_report
    print("(j) pink_lfp w0=%g: predicted worst %.2e, rerouted %d" % (w0, rep["worst"], rep["rerouted"]))
    assert rep["watched"] and rep["rerouted"] == 0, rep
    _check("j", "pink_lfp w0=%g" % w0, cwt.coefficients, truth(x, FS, cwt.frequencies, w0, threads=8), "complex")


def test_j_exact_precision_under_a_drift():
    """precision = 'exact' on drift1000 at w0 = 5: what is achievable there."""
    from ghost_amd.wave import ContinuousWaveletTransform, Morlet
    n, w0 = 120000, 5.0
    x = _steep("drift1000", n)
    cwt = ContinuousWaveletTransform(wavelet=Morlet(w0=w0))
    cwt.transform(x, fs=FS, output="complex", precision="exact")
    assert not levels(cwt._plan)
    _check("j", "drift1000 w0=5 precision='exact'", cwt.coefficients, truth(x, FS, cwt.frequencies, w0, threads=8),
           "complex")
