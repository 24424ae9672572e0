"""transform() / CwtPlan at the channel counts where grids and batches change (GPU): the 32-slot line of the
interpolating synthesis' grid order, epoch batches times channels, the 65535-slot launch limit and the 65535-row split,
the other paths above 32 slots, precision='auto' with one bad electrode far from channel 0, and coupling() / triggered()
beyond one placement group.  tests/channel_cases.py builds the recordings -- every channel a power of two times one of
five base signals, so the oracle runs on five -- and tests/test_channel_cases_cpu.py pins the planner's decisions.

Three assertions on every case, over every channel, row and column:
1. the oracle gate: conftest.rel_err per row below TOL = 1e-5 (2 TOL on power);
2. homogeneity: channels of one base agree bit for bit once their power of two is taken out;
3. independence of the channel count: channels 0, C // 2 and C - 1 carry the bits of a one-channel plan with the same
   arguments run on that channel alone.

Every step of the pipeline commuted with the power-of-two scale on the MI355X: no row needed the weaker form of 2."""
import functools
import time

import numpy as np
import pytest

import channel_cases as cc
import triggered_model as tm

pytestmark = pytest.mark.gpu


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def _base(n, seed=1234):
    return _frozen(cc.base_signals(n, seed))


@functools.lru_cache(maxsize=None)
def _reference(case):
    """complex128 (5, S, n) of a case's five base signals, made once."""
    if case == "A":
        return _frozen(cc.oracle_base(_base(cc.A_N), cc.A_F))
    if case == "A folded":
        return _frozen(_reference("A")[:, 1:])
    if case == "B":
        return _frozen(cc.oracle_base(_base(cc.B_N), cc.B_F, epoch_bounds=cc.B_EPOCHS))
    if case in ("C limit", "C rows"):
        lay = cc.C_LIMIT if case == "C limit" else cc.C_ROWS
        return _frozen(cc.oracle_base(_base(lay["n"]), cc.C_F, epoch_bounds=lay["epochs"]))
    if case == "D":
        return _frozen(cc.oracle_base(_base(cc.D_N), cc.D_F, epoch_bounds=cc.D_EPOCHS, gamma=3, beta=3))
    if case == "D morlet":
        import morlet_model
        return _frozen(np.stack([morlet_model.cwt_decimated(b, cc.FS, cc.morlet_freqs(), cc.D_MORLET_W0)
                                 for b in _base(cc.D_MORLET_N)]))
    if case == "F":
        return _frozen(cc.oracle_base(_base(cc.F_N, 11), cc.F_F))
    raise KeyError(case)


def _plan(c, n, f, **kw):
    from ghost_amd.engine import CwtPlan
    return CwtPlan(n, c, cc.FS, f, **kw)


def _check(tag, x, got, ref, f, output, one_channel=True, **kw):
    """The three assertions on ``got`` = the plan's result for the recording ``x``; ``ref``: the five bases' complex
    rows; ``kw``: the plan's arguments, for the one-channel plans.  -> the worst oracle error."""
    n_ch, n = x.shape
    assert got.shape[:2] == (n_ch, len(f))
    err = cc.oracle_error(got, cc.as_output(output, ref), output)
    assert err.shape == (n_ch, len(f))
    same = cc.homogeneous(got, output)
    print("%s C=%d %s: worst oracle error %.3g (gate %.0e) at channel %d row %d; homogeneous: %s"
          % ((tag, n_ch, output, err.max(), cc.gate(output)) + np.unravel_index(err.argmax(), err.shape) + (same,)))
    assert err.max() < cc.gate(output), (tag, n_ch, output, err.max())
    assert same, (tag, n_ch, output)
    if one_channel:
        for c in cc.picks(n_ch):
            p1 = _plan(1, n, f, output=output, **kw)
            np.testing.assert_array_equal(p1.execute(x[c:c + 1])[0], got[c], err_msg="%s C=%d channel %d alone" % (tag, n_ch, c))
            p1.close()
    return float(err.max())


# ---- A. the 32-slot line and the interpolating kernels -----------------------------------------------------------------
@pytest.mark.parametrize("c, output", [(32, "amplitude"), (33, "amplitude"), (40, "amplitude"), (33, "complex"), (33, "power")])
def test_a_both_sides_of_the_32_slot_line(c, output):
    """k_synthi's grid runs channels-fastest up to 32 slots and items-fastest above; its item list is cut by C too."""
    x = cc.expand(_base(cc.A_N), c)
    p = _plan(c, cc.A_N, cc.A_F, output=output)
    got = p.execute(x)
    p.close()
    _check("A", x, got, _reference("A"), cc.A_F, output)


def _grid_orders(option, c, stride):
    """(x, the default's result, the rows of the k_synth7 / k_synth7s levels) of case A at ``stride``, after
    interp_grid = 0 (items fastest) and 1 (channels fastest) have given the default's bits."""
    x = cc.expand(_base(cc.A_N), c)
    results = {}
    for grid in (None, 0, 1):
        option("interp_grid", grid)
        p = _plan(c, cc.A_N, cc.A_F, output_stride=stride)
        assert p.info["n_interp"] == 9
        results[grid] = p.execute(x)
        plain = [lv["decimation"] for lv, it in zip(p.debug_levels(), p.debug_interp()["levels"]) if it is None]
        synth7 = np.isin(p.scale_info()["decimation"], plain) & (p.scale_info()["method"] == 0)
        p.close()
    option("interp_grid", None)
    np.testing.assert_array_equal(results[0], results[None])
    np.testing.assert_array_equal(results[1], results[None])
    assert plain == [2, 4, 8] and synth7.tolist() == [False] + [True] * 6 + [False] * 9
    return x, results[None], synth7


@pytest.mark.parametrize("c", [8, 40])
def test_a_either_grid_order_gives_the_same_bits(option, c):
    """interp_grid = 0 and 1 forced on both sides of the 32-slot line at full rate (k_synthi): the default's bits."""
    x, got, _ = _grid_orders(option, c, 1)
    _check("A grid orders", x, got, _reference("A"), cc.A_F, "amplitude", one_channel=False)


SYNTH7_TOL = 2.5e-7             # tests/test_gpu_output_stride_matrix.py: k_synth7s amplitude rows against k_synth7's


def test_a_output_stride_4_at_40_channels(option):
    """output_stride = 4 at 40 channels (k_synthis, k_synth7s), either grid order: the three assertions on the strided
    result; the rows of the time-domain scale and of the interpolated levels (k_synthis) are the full-rate rows' every
    fourth column bit for bit, the amplitude rows of the k_synth7s levels within the two last-place units of the row's
    peak that tests/test_gpu_output_stride_matrix.py holds them to (the next test asks for their bits)."""
    x, got, synth7 = _grid_orders(option, 40, 4)
    full = _plan(40, cc.A_N, cc.A_F)
    want = full.execute(x)[..., ::4]
    full.close()
    np.testing.assert_array_equal(got[:, ~synth7], want[:, ~synth7])
    diff = np.abs(got[:, synth7].astype(np.float64) - want[:, synth7]).max(axis=-1) / np.abs(want[:, synth7]).max(axis=-1)
    print("A stride 4 C=40: k_synth7s rows differ from k_synth7's by %.3g of the row's peak (bound %.1e)" % (diff.max(), SYNTH7_TOL))
    assert diff.max() <= SYNTH7_TOL
    _check("A stride 4", x, got, _reference("A")[..., ::4], cc.A_F, "amplitude", output_stride=4)


def test_a_output_stride_4_k_synth7s_rows_bit_for_bit(option):
    """The rows of the levels R = 2, 4, 8 at output_stride = 4 (k_synth7s) against the full-rate rows' (k_synth7) every
    fourth column, bit for bit, at 40 channels.

    This test found 48 528 of the 1 200 000 elements of these six rows (4.0 %; the same share at 8 channels) one or two
    units in the last place apart, 1.21e-7 of the row's peak: the compiler fused the real twiddles of the last radix-16
    layer into the butterfly's adds in k_synth7's |.| instantiations and not in k_synth7s's.  Both kernels now multiply
    them as written (synth_math.h: idft16v<true>; DESIGN.md, "Output stride")."""
    x, got, synth7 = _grid_orders(option, 40, 4)
    full = _plan(40, cc.A_N, cc.A_F)
    want = full.execute(x)[..., ::4]
    full.close()
    wrong = got[:, synth7] != want[:, synth7]
    print("A stride 4 C=40: %d of %d elements of the k_synth7s rows differ from k_synth7's, by at most %.3g"
          % (wrong.sum(), wrong.size, np.abs(got[:, synth7].astype(np.float64) - want[:, synth7]).max()))
    np.testing.assert_array_equal(got[:, synth7], want[:, synth7])


def test_a_channel_sums_inside_the_forward_pass_at_33_channels(option):
    """Case A without its one time-domain scale, so that the forward column pass takes the channel sums (api.cpp:
    fold_mean needs a plan without direct scales): the three assertions on the folded plan, and fold_mean = 0 within the
    2e-6 of test_channel_means_taken_inside_the_forward_passes."""
    from conftest import rel_err
    c, f = 33, cc.A_F[1:]
    x = cc.expand(_base(cc.A_N), c)
    p = _plan(c, cc.A_N, f, output="complex")
    assert np.all(p.scale_info()["method"] == 0)
    got = p.execute(x)
    assert p.debug_mean_folded()
    p.close()
    _check("A folded", x, got, _reference("A folded"), f, "complex")
    option("fold_mean", 0)
    q = _plan(c, cc.A_N, f, output="complex")
    plain = q.execute(x)
    assert not q.debug_mean_folded()
    q.close()
    diff = rel_err(got.reshape(-1, cc.A_N), plain.reshape(-1, cc.A_N)).max()
    print("A folded C=33: fold_mean = 0 differs by %.3g (bound 2e-6)" % diff)
    assert diff < 2e-6
    _check("A fold_mean = 0", x, plain, _reference("A folded"), f, "complex")


# ---- B. epoch batches times channels -------------------------------------------------------------------------------------
@pytest.mark.parametrize("c, batch_bytes", [(3, None), (33, None), (4369, cc.B_BATCH_BYTES), (4370, cc.B_BATCH_BYTES)])
def test_b_epoch_batches_times_channels(option, c, batch_bytes):
    """Twenty short epochs launched as extra channels: 48 and 528 slots; 4369 x 15 = 65535 slots exactly and 4370 x 14,
    the two sides of the batch cap 65535 / C and of the time-domain path's flush.  Every epoch its own 'same'
    convolution, zero outside, and a block request across the batch boundary equals the slice."""
    t0 = time.perf_counter()
    if batch_bytes is not None:
        option("batch_bytes", batch_bytes)
    x = cc.expand(_base(cc.B_N), c)
    p = _plan(c, cc.B_N, cc.B_F, epoch_bounds=cc.B_EPOCHS)
    first = p.debug_batches()[0][1]
    assert first == min(16, 65535 // c)
    got = p.execute(x)
    t1 = time.perf_counter()
    _check("B", x, got, _reference("B"), cc.B_F, "amplitude", epoch_bounds=cc.B_EPOCHS)
    gaps = ~cc.inside(cc.B_N, cc.B_EPOCHS)
    assert not got[:, :, gaps].any()                          # samples of no epoch (transforms.py:185)
    assert np.all(got[:, :, ~gaps].max(axis=2) > 0)
    a, length = cc.b_block(first)
    np.testing.assert_array_equal(p.execute_block(x, a, length), got[:, :, a:a + length])
    p.close()
    print("B C=%d: device and copies %.1f s, checks %.1f s" % (c, t1 - t0, time.perf_counter() - t1))


# ---- C. the limit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["C limit", "C rows"])
def test_c_channel_limit_and_rows_beyond_one_grid(case):
    """65535 channels (the plan's limit; 3 x 65535 rows) and 21846 (65535 + 3 rows), device-resident into a buffer full
    of a non-zero pattern: the columns between the epochs are exactly 0 in every row (launch_zero_range, split into
    calls of 65535 rows), everything else is the transform."""
    from ghost_amd._lib import lib, check
    from ghost_amd.engine import DeviceBuffer
    t0 = time.perf_counter()
    lay = cc.C_LIMIT if case == "C limit" else cc.C_ROWS
    c, n, eb = lay["n_channels"], lay["n"], lay["epochs"]
    x = cc.expand(_base(n), c)
    p = _plan(c, n, cc.C_F, epoch_bounds=eb)
    assert p.info["out_bytes"] == c * 3 * n * 4
    xb, ob = DeviceBuffer(x.nbytes), DeviceBuffer(p.info["out_bytes"])
    xb.upload(x)
    check(lib.gcwt_device_memset(ob.ptr, 0x55, ob.nbytes))              # every float 1.47e13
    assert np.all(ob.download((3, n), np.float32) == np.frombuffer(b"\x55" * 4, np.float32)[0])
    p.execute_device(xb, ob)
    got = ob.download((c, 3, n), np.float32)
    xb.free(); ob.free()
    t1 = time.perf_counter()
    gaps = ~cc.inside(n, eb)
    assert gaps.sum() == 50 * (len(eb) - 1)
    assert not got[:, :, gaps].any()
    assert np.all(got[:, :, ~gaps].max(axis=2) > 0) and np.all(got < 1e6)
    _check(case, x, got, _reference(case), cc.C_F, "amplitude", epoch_bounds=eb)
    p.close()
    print("%s C=%d: device and copies %.1f s, checks %.1f s" % (case, c, t1 - t0, time.perf_counter() - t1))


def test_c_one_channel_more_is_refused():
    from ghost_amd import _lib
    with pytest.raises(_lib.GhostCwtError) as e:
        _plan(65536, 600, cc.C_F)
    assert e.value.code == _lib.ERR_UNSUPPORTED


# ---- D. the other paths above 32 slots -----------------------------------------------------------------------------------
@pytest.mark.parametrize("blockconv", [1, 0])
def test_d_time_domain_block_convolution_and_full_band_at_80_slots(option, blockconv):
    from ghost_amd import _lib
    if not blockconv:
        option("blockconv", 0)
    kw = dict(gamma=3, beta=3, epoch_bounds=cc.D_EPOCHS)
    x = cc.expand(_base(cc.D_N), 40)
    p = _plan(40, cc.D_N, cc.D_F, output="complex", **kw)
    want = [_lib.SCALE_DIRECT, _lib.SCALE_BLOCKCONV] if blockconv else [_lib.SCALE_DIRECT, _lib.SCALE_FULLBAND]
    assert sorted(set(p.scale_info()["method"].tolist())) == want
    got = p.execute(x)
    p.close()
    _check("D blockconv" if blockconv else "D full band", x, got, _reference("D"), cc.D_F, "complex", **kw)
    assert not got[:, :, ~cc.inside(cc.D_N, cc.D_EPOCHS)].any()


@pytest.mark.parametrize("output", ["complex", "amplitude"])
def test_d_morlet_at_40_channels(output):
    """Morlet(w0 = 6) from the time-domain scales down to decimation 64, against the float64 model of the Morlet path
    (tests/morlet_model.py: cwt_decimated) on the five bases."""
    f = cc.morlet_freqs()
    x = cc.expand(_base(cc.D_MORLET_N), 40)
    p = _plan(40, cc.D_MORLET_N, f, output=output, morlet_w0=cc.D_MORLET_W0)
    assert p.scale_info()["decimation"].max() >= 16
    got = p.execute(x)
    p.close()
    _check("D Morlet", x, got, _reference("D morlet"), f, output, morlet_w0=cc.D_MORLET_W0)


# ---- E. precision='auto', one bad electrode far from channel 0 -----------------------------------------------------------
def test_e_one_bad_electrode_at_channel_37_of_40():
    """The recording and line of test_one_bad_electrode_pays_for_one at 40 channels and 12 scales: with the line (300 x
    the channel's spread) on channel 37 alone, that channel's flagged scales are made again by the exact paths and the
    other 39 keep precision='high''s bits; with it on channels 3..39 every channel is made again.  The three
    assertions hold throughout (homogeneity among the channels of one source: a clean or a dirty base); the
    one-channel plans are 'auto' plans too, on the clean picks 0, 20, 39 of the first recording."""
    from oracle import ghost_oracle as orc
    t0 = time.perf_counter()
    n, c, f = cc.E_N, 40, cc.E_F
    base = _base(n)
    for dirty in ([37], list(range(3, 40))):
        x, sources, src = cc.bad_electrodes(base, c, dirty)
        used = np.unique(src)
        ref = np.zeros((10, len(f), n))
        for s in used:
            ref[s] = orc.cwt_amplitude(sources[s].astype(np.float64), cc.FS, f, n_threads=8)
        ph = _plan(c, n, f, precision="high")
        high = ph.execute(x)
        ph.close()
        p = _plan(c, n, f, precision="auto")
        got = p.execute(x)
        rep = p.precision_report()
        p.close()
        err = cc.oracle_error(got, ref, "amplitude", source=src)
        differs = (got != high).any(axis=(1, 2))
        print("E line on %d channels: rerouted %d scales, worst oracle error %.3g (dirty %.3g), %d channels differ from 'high'"
              % (len(dirty), rep["rerouted"], err.max(), err[dirty].max(), differs.sum()))
        assert rep["rerouted"] > 0
        assert err.max() < cc.TOL, (dirty, np.unravel_index(err.argmax(), err.shape))
        assert cc.homogeneous(got, "amplitude", source=src)
        if len(dirty) == 1:
            assert differs.tolist() == [ch in dirty for ch in range(c)]
            for ch in cc.picks(c):
                p1 = _plan(1, n, f, precision="auto")
                np.testing.assert_array_equal(p1.execute(x[ch:ch + 1])[0], got[ch], err_msg="channel %d alone" % ch)
                p1.close()
        else:
            assert differs.all()
    print("E: %.1f s" % (time.perf_counter() - t0))


# ---- F. coupling() and triggered() beyond one placement group ------------------------------------------------------------
def _resident_case_f(c):
    x = cc.expand(_base(cc.F_N, 11), c)
    plan = _plan(c, cc.F_N, cc.F_F, output="complex")
    result = plan.execute_resident(x)
    w = result.to_host(np.complex64)
    _check("F", x, w, _reference("F"), cc.F_F, "complex", one_channel=False)
    return x, plan, result, w


def _alone(x, w):
    """Yields (c, a resident result that holds channel c only), its rows checked against the C-channel result's."""
    one = _plan(1, cc.F_N, cc.F_F, output="complex")
    r1 = None
    for c in range(x.shape[0]):
        r1 = one.execute_resident(x[c:c + 1], result=r1)
        np.testing.assert_array_equal(r1.to_host(np.complex64)[0], w[c], err_msg="channel %d alone" % c)
        yield c, r1
    r1.free()
    one.close()


@pytest.mark.parametrize("c", [9, 33])
def test_f_coupling_beyond_one_placement_group(c):
    """Units (channel, run) are dealt in groups of eight, the last one padded (resident_op.h): 9 and 33 channels.  The
    kernel against the float64 model on its own input within the derived bounds of tests/test_gpu_coupling.py, and every
    channel's cells are the cells of a call on a result that holds that channel alone."""
    import test_gpu_coupling as tc
    x, plan, result, w = _resident_case_f(c)
    cells = ((3, 3), (0, 4), 64), ((0, 6), (0, 6), 1000)
    company = []
    for ph, am, window in cells:
        company.append(tc._run(result, ph, am, window))
        tc._compare(company[-1], w, ph, am, window, "F C=%d" % c)
    for ch, r1 in _alone(x, w):
        for (ph, am, window), together in zip(cells, company):
            alone = tc._run(r1, ph, am, window)
            for name in ("vector", "mvl", "amplitude"):
                np.testing.assert_array_equal(alone[name][0], together[name][ch], err_msg="%s of channel %d" % (name, ch))
    result.free()
    plan.close()


@pytest.mark.parametrize("c", [9, 33])
def test_f_triggered_beyond_one_placement_group(c):
    """As above for triggered(): against tests/triggered_model.py within the bounds of tests/test_gpu_triggered.py, and
    alone = in company, bit for bit."""
    import test_gpu_triggered as tg
    x, plan, result, w = _resident_case_f(c)
    rng = np.random.default_rng(17)
    calls = [(tg._events(67, 31, 32, cc.F_N, rng), 31, 32, None), (tg._events(5, 100, 163, cc.F_N, rng), 100, 163, (1, 4))]
    company = []
    for cols, nb, na, rows in calls:
        company.append(tg._run(result, cols, nb, na, rows))
        ref = tm.model(w, cols, nb, na)
        tg._compare(company[-1], ref if rows is None else tg._rows_of(ref, *rows), len(cols), "F C=%d" % c)
    for ch, r1 in _alone(x, w):
        for (cols, nb, na, rows), together in zip(calls, company):
            alone = tg._run(r1, cols, nb, na, rows)
            for name in tg.NAMES:
                np.testing.assert_array_equal(alone[name][0], together[name][ch], err_msg="%s of channel %d" % (name, ch))
    result.free()
    plan.close()
