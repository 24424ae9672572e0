"""The channel-count cases without a device (tests/channel_cases.py): the recordings tell every channel apart and their
expected rows are the oracle's, and the planner puts every case on the branch it is there for -- FFT length, methods,
decimations, interpolated levels, launch batches, sizes.  A planner change that moves a case off its branch fails here,
not silently in tests/test_gpu_channel_matrix.py."""
import numpy as np
import pytest

import channel_cases as cc
from oracle import ghost_oracle as orc


def _plan(n, c, f, **kw):
    from ghost_amd.engine import CwtPlan
    return CwtPlan(n, c, cc.FS, f, **kw)


# ---- the helper ----------------------------------------------------------------------------------------------------
def test_every_channel_is_an_exact_power_of_two_of_its_base():
    base = cc.base_signals(3001)
    x = cc.expand(base, 200)
    k, s = cc.exponents(200)
    assert x.dtype == np.float32 and x.shape == (200, 3001)
    assert k.min() == -4 and k.max() == 4 and set(s.tolist()) == {-1, 1}
    np.testing.assert_array_equal(x.astype(np.float64), base[np.arange(200) % 5].astype(np.float64) * (s * 2.0 ** k)[:, None])
    # the channel the others are compared with: k = 0, s = +1 is the base itself
    home = np.flatnonzero((k == 0) & (s == 1))
    assert home[:5].tolist() == [20, 21, 22, 23, 24]
    np.testing.assert_array_equal(x[home[:5]], base)
    # far from float32's denormals and its overflow
    assert np.abs(x[x != 0]).min() > 1e-12 and np.abs(x).max() < 1e3


def test_no_two_channels_of_a_period_alike_and_no_tile_meets_its_copy():
    x = cc.expand(cc.base_signals(257), 4 * cc.PERIOD)
    first = x[:cc.PERIOD]
    assert len({row.tobytes() for row in first}) == cc.PERIOD
    np.testing.assert_array_equal(x[cc.PERIOD:2 * cc.PERIOD], first)
    # channels c and c + 90 hold the same data; 90 is odd x 2: the copy never sits at the same place of a tile
    for tile in (8, 16, 32, 64):
        assert cc.PERIOD % tile != 0 and all(c % tile != (c + cc.PERIOD) % tile for c in range(tile))


def test_factors_by_output_mode():
    k, s = cc.exponents(100)
    np.testing.assert_array_equal(cc.factors(100, "complex"), s * 2.0 ** k)
    np.testing.assert_array_equal(cc.factors(100, "amplitude"), 2.0 ** k)
    np.testing.assert_array_equal(cc.factors(100, "power"), 4.0 ** k)
    assert cc.factors(100, "complex")[52] == -2.0 ** -3 and cc.factors(100, "power")[37] == 64.0


@pytest.mark.parametrize("output", ["complex", "amplitude", "power"])
def test_expected_rows_are_the_oracle_on_the_expanded_channels(output):
    """The oracle run directly on a few expanded channels, epochs included (mean removal over the whole recording is
    linear): the scaled base rows are those rows -- to float64 rounding at most; measured 0.0."""
    n, f, eb = 6000, [250.0, 60.0, 11.0], [[0, 2500], [2600, 6000]]
    base = cc.base_signals(n)
    x = cc.expand(base, 100)
    exp = cc.expected(cc.oracle_base(base, f, output, eb), 100, output)
    assert exp.shape == (100, 3, n)
    for c in (0, 7, 24, 37, 52, 99):
        direct = cc.as_output(output, orc.cwt_complex(x[c].astype(np.float64), cc.FS, f, np.array(eb)))
        err = np.abs(direct - exp[c]).max() / np.abs(direct).max()
        assert err <= 1e-15, (output, c, err)


@pytest.mark.parametrize("output", ["complex", "amplitude", "power"])
def test_the_vectorised_checks_see_what_they_should(output):
    """unscaled / homogeneous / oracle_error on a made-up result: exact on the expected rows themselves, and one wrong
    bit, two channels swapped or a wrong stride are all seen."""
    rng = np.random.default_rng(3)
    ref = rng.standard_normal((5, 2, 40)) + (1j * rng.standard_normal((5, 2, 40)) if output == "complex" else 0)
    ref = np.abs(ref) if output != "complex" else ref
    ref32 = ref.astype(np.complex64 if output == "complex" else np.float32)
    for n_ch in (3, 8, 33, 97):
        got = (ref32[cc.base_index(n_ch)] * cc.factors(n_ch, output).astype(np.float32)[:, None, None]).astype(ref32.dtype)
        assert cc.homogeneous(got, output)
        np.testing.assert_array_equal(cc.unscaled(got, output), ref32[cc.base_index(n_ch)])
        err = cc.oracle_error(got, ref, output)
        want = np.stack([np.abs(got[c].astype(ref.dtype) - cc.expected(ref, n_ch, output)[c]).max(axis=-1) /
                         np.abs(cc.expected(ref, n_ch, output)[c]).max(axis=-1) for c in range(n_ch)])
        assert err.shape == (n_ch, 2)
        np.testing.assert_array_equal(err, want)
        assert err.max() < 1e-7
        if n_ch <= 5:
            continue
        bad = got.copy()
        flat = bad.view(np.float32)
        flat[n_ch - 1, 1, 7] = np.nextafter(flat[n_ch - 1, 1, 7], np.float32(np.inf))
        assert not cc.homogeneous(bad, output)
        swapped = got.copy()
        swapped[[5, 6]] = swapped[[6, 5]]
        assert not cc.homogeneous(swapped, output) and cc.oracle_error(swapped, ref, output).max() > 0.1


def test_bad_electrodes_are_scaled_dirty_bases():
    base = cc.base_signals(5000)
    x, sources, src = cc.bad_electrodes(base, 40, [37])
    clean = cc.expand(base, 40)
    keep = np.arange(40) != 37
    np.testing.assert_array_equal(x[keep], clean[keep])
    assert src[37] == 7 and src[keep].max() < 5
    np.testing.assert_array_equal(x[37], sources[7] * np.float32(8.0))
    assert np.abs(x[37]).max() > 250 * clean[37].std()          # the line: 300 x the spread under a sin^2 window
    x, sources, src = cc.bad_electrodes(base, 40, list(range(3, 40)))
    assert src[:3].tolist() == [0, 1, 2] and src[3:].min() >= 5


# ---- the planner's decisions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 8, 32, 33, 40])
def test_case_a_reaches_every_interpolated_level(c):
    p = _plan(cc.A_N, c, cc.A_F)
    si = p.scale_info()
    assert p.info["fft_length"] == 32768 and p.segments() == [(0, cc.A_N, 32768)]
    assert si["method"].tolist() == [1] + [0] * 15
    assert sorted(set(si["decimation"][1:].tolist())) == [2, 4, 8, 16, 32, 64, 128]
    interp = {lv["decimation"]: None if it is None else (it["q"], it["factor"])
              for lv, it in zip(p.debug_levels(), p.debug_interp()["levels"])}
    assert interp == {2: None, 4: None, 8: None, **cc.A_INTERP}
    assert p.debug_batches() == [(0, 1)]                      # slots = C: 32 is the last channels-fastest count
    q = _plan(cc.A_N, c, cc.A_F, output_stride=4)
    assert q.info["n_interp"] == p.info["n_interp"] == 9 and q.out_shape == (c, 16, 5000)


@pytest.mark.parametrize("c, batch_bytes, batches", [(1, None, [(0, 16), (16, 4)]), (3, None, [(0, 16), (16, 4)]),
                                                     (33, None, [(0, 16), (16, 4)]),
                                                     (1, cc.B_BATCH_BYTES, [(0, 16), (16, 4)]),
                                                     (4369, cc.B_BATCH_BYTES, [(0, 15), (15, 5)]),
                                                     (4370, cc.B_BATCH_BYTES, [(0, 14), (14, 6)])])
def test_case_b_batches_on_both_sides_of_the_grid_limit(option, c, batch_bytes, batches):
    if batch_bytes is not None:
        option("batch_bytes", batch_bytes)
    p = _plan(cc.B_N, c, cc.B_F, epoch_bounds=cc.B_EPOCHS)
    si = p.scale_info()
    assert all(seg[2] == 4096 for seg in p.segments()) and len(p.segments()) == 20
    assert si["method"].tolist() == [1, 0, 0] and si["decimation"].tolist() == [1, 4, 4]
    assert p.debug_batches() == batches
    # 65535 / C epochs per batch, and the direct path's launches flushed at the same count (pipeline.cpp: (ne + 1) C > 65535)
    assert batches[0][1] == min(16, 65535 // c)
    assert p.info["out_bytes"] == c * 3 * cc.B_N * 4
    if c >= 4369:
        assert 6.5e9 < p.info["workspace_bytes"] < 7.5e9 and 0.38e9 < p.info["out_bytes"] < 0.43e9
    # the block request of the device test cuts the boundary between the two batches
    first = batches[0][1]
    a, length = cc.b_block(first)
    assert cc.B_EPOCHS[first - 1][0] < a < cc.B_EPOCHS[first - 1][1] and cc.B_EPOCHS[first + 1][0] < a + length <= cc.B_N


@pytest.mark.parametrize("case, batches, rows", [(cc.C_LIMIT, [(0, 1), (1, 1)], 3 * 65535), (cc.C_ROWS, [(0, 2), (2, 2)], 65535 + 3)])
def test_case_c_rows_beyond_one_grid(case, batches, rows):
    p = _plan(case["n"], case["n_channels"], cc.C_F, epoch_bounds=case["epochs"])
    si = p.scale_info()
    assert all(seg[2] == 4096 for seg in p.segments())
    assert si["method"].tolist() == [0, 0, 1] and si["decimation"].tolist() == [4, 4, 1]
    assert p.debug_batches() == batches
    assert case["n_channels"] * len(cc.C_F) == rows and p.info["out_bytes"] == rows * case["n"] * 4
    assert p.info["workspace_bytes"] < 7.5e9
    gaps = ~cc.inside(case["n"], case["epochs"])
    assert gaps[250:300].all() and gaps.sum() == 50 * (len(case["epochs"]) - 1)


def test_one_channel_more_than_the_limit_is_refused():
    from ghost_amd import _lib
    with pytest.raises(_lib.GhostCwtError, match="UNSUPPORTED|n_channels") as e:
        _plan(600, 65536, cc.C_F)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    assert _plan(600, 65535, cc.C_F).n_channels == 65535


def test_case_d_methods(option):
    from ghost_amd import _lib
    kw = dict(gamma=3, beta=3, epoch_bounds=cc.D_EPOCHS, output="complex")
    p = _plan(cc.D_N, 40, cc.D_F, **kw)
    assert sorted(set(p.scale_info()["method"].tolist())) == [_lib.SCALE_DIRECT, _lib.SCALE_BLOCKCONV]
    assert p.info["n_blockconv"] == 4 and p.debug_batches() == [(0, 2)]            # 80 slots
    option("blockconv", 0)
    q = _plan(cc.D_N, 40, cc.D_F, **kw)
    assert sorted(set(q.scale_info()["method"].tolist())) == [_lib.SCALE_DIRECT, _lib.SCALE_FULLBAND]
    assert q.info["n_fullband"] == 2 and q.info["n_blockconv"] == 0 and q.debug_batches() == [(0, 2)]


def test_case_d_morlet_levels():
    f = cc.morlet_freqs()
    p = _plan(cc.D_MORLET_N, 40, f, morlet_w0=cc.D_MORLET_W0, output="complex")
    si = p.scale_info()
    assert f.size == 23 and si["decimation"].max() >= 16
    assert sorted(set(si["decimation"].tolist())) == [1, 2, 4, 8, 16, 32, 64]
    assert (si["method"] == 1).sum() == 2 and (si["method"] == 0).sum() == 21


def test_cases_e_and_f_layouts():
    p = _plan(cc.E_N, 40, cc.E_F, precision="auto")
    assert p.info["fft_length"] == 262144 and np.all(p.scale_info()["method"] == 0)
    assert p.precision_report()["watched"]
    for c in (9, 33):                                         # two and five placement groups of 8 units, the last padded
        q = _plan(cc.F_N, c, cc.F_F, output="complex")
        assert q.info["fft_length"] == 16384 and np.all(q.scale_info()["method"] == 0)
        assert c % 8 == 1
