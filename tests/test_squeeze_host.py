"""squeeze() without a GPU: the cells, the models of the definition against a plain loop and against each other, the
condition of the end-to-end test on the oracle's own coefficients (how many entries the float64 model cannot decide, how
sharp the squeezed result is), the C entry point's argument checks, and the refusals of the class and the engine.  The device
side: tests/test_gpu_squeeze.py."""
import ctypes as C

import numpy as np
import pytest

import ridge_model as rm
import squeeze_model as sm

FS = 1000.0


# -- the cells -------------------------------------------------------------------------------------------------------------
def test_edges_are_geometric_midpoints_with_half_a_step_at_either_end():
    from ghost_amd.engine import squeeze_edges
    f = np.array([10.0, 20.0, 80.0])
    edges, descending = squeeze_edges(f)
    assert edges.dtype == np.float32 and edges.shape == (4,) and descending is False
    want = np.array([10.0 / np.sqrt(2.0), np.sqrt(200.0), 40.0, 160.0])
    assert np.array_equal(edges, want.astype(np.float32))
    back, desc = squeeze_edges(f[::-1])
    assert desc is True and np.array_equal(back, edges)                     # the edges ascend either way
    grid = np.geomspace(20.0, 100.0, 38)
    edges, _ = squeeze_edges(grid)
    assert np.all(np.diff(edges) > 0) and np.all(edges[:-1] < grid) and np.all(grid < edges[1:])
    ratio = edges[1:].astype(np.float64) / edges[:-1]
    assert np.allclose(ratio, ratio[0], rtol=1e-6)                          # a geometric grid has cells of one width
    assert squeeze_edges([3, 4])[0].shape == (3,)
    assert squeeze_edges(np.geomspace(1.0, 2.0, 4096))[0].shape == (4097,)


def test_edges_refuse_what_they_cannot_use():
    from ghost_amd.engine import squeeze_edges
    for bad in ([], [10.0], 10.0):
        with pytest.raises(ValueError, match="at least 2"):
            squeeze_edges(bad)
    for bad in ([10.0, np.nan], [0.0, 1.0], [-1.0, 1.0], [1.0, np.inf]):
        with pytest.raises(ValueError, match="finite and positive"):
            squeeze_edges(bad)
    for bad in ([1.0, 2.0, 2.0], [1.0, 3.0, 2.0], [2.0, 2.0]):
        with pytest.raises(ValueError, match="monotonic"):
            squeeze_edges(bad)
    with pytest.raises(ValueError, match="at most 4096"):
        squeeze_edges(np.geomspace(1.0, 2.0, 4097))
    # distinct in float64, one float32 after the cast: the message names the pair
    close = np.array([10.0, 20.0, 20.0 * (1 + 1e-9), 20.0 * (1 + 2e-9), 40.0])
    with pytest.raises(ValueError, match=r"centres 2 and 3 .*too close"):
        squeeze_edges(close)
    with pytest.raises(ValueError, match=r"centres 1 and 2 .*too close"):
        squeeze_edges(close[::-1])
    with pytest.raises(ValueError, match="float32's range"):
        squeeze_edges([1e-60, 1e-50])


# -- the models ------------------------------------------------------------------------------------------------------------
def _random(c, s, n, seed):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((c, s, n)) + 1j * rng.standard_normal((c, s, n))).astype(np.complex64)
    w[..., n // 3:n // 3 + n // 5] = 0
    g = rng.standard_normal(s).astype(np.float32)
    floor2 = (0.8 * rng.random(s)).astype(np.float32)                       # |w|^2 is exponential with mean 2: a third is out
    return w, g, floor2, (2.5 * np.pi * rng.random(s)).astype(np.float32)


@pytest.mark.parametrize("descending", [False, True])
def test_the_model_is_the_definition_entry_by_entry(descending):
    w, g, floor2, nu = _random(2, 7, 60, 11)
    seg = [(0, 6), (6, 7), (7, 30), (30, 60)]
    edges = np.array([3.0, 20.0, 35.0, 60.0, 110.0, 200.0], np.float32)     # hz = 250: frequencies reach from 0 to 312
    for rows in ((0, 7), (2, 1), (1, 5)):
        got = sm.model(w, rows, g, floor2, nu, 250.0, seg, edges, descending)
        freq, index, z = sm.brute(w, rows, g, floor2, nu, 250.0, seg, edges, descending)
        assert np.array_equal(np.isnan(got["frequency"]), np.isnan(freq))
        live = ~np.isnan(freq)
        assert np.abs(got["frequency"][live] - freq[live]).max() <= 1e-9
        assert np.array_equal(got["index"], index)
        assert np.abs(got["coefficients"] - z).max() <= 1e-12 and np.array_equal(got["power"], np.abs(got["coefficients"]) ** 2)
        assert np.any(index == -1) and set(np.unique(index).tolist()) <= set(range(-1, 5))
        assert rows[1] < 5 or set(np.unique(index).tolist()) == set(range(-1, 5))
        gap = slice(20, 32)
        assert np.all(index[..., gap] == -1) and not np.any(got["coefficients"][..., gap]) and np.all(np.isnan(freq[..., gap]))
        assert np.all(np.isnan(freq[..., 6]))                               # a segment of one column
        # the frequency is ridge_model's on every row and does not know the threshold
        again = sm.model(w, rows, g, np.zeros(7, np.float32), nu, 250.0, seg, edges, descending)
        assert np.array_equal(again["frequency"], got["frequency"], equal_nan=True)
        one = rm.frequency64(w, np.full((2, 1, 60), rows[0], np.int32), nu, 250.0, seg)["frequency"]
        assert np.array_equal(one[:, 0], got["frequency"][:, 0], equal_nan=True)


def test_the_float32_steps_are_the_definition_up_to_rounding():
    w, g, floor2, nu = _random(3, 9, 300, 5)
    seg, rows = [(0, 100), (100, 101), (101, 300)], (1, 7)
    edges = np.geomspace(5.0, 300.0, 12).astype(np.float32)
    ref = sm.model(w, rows, g, floor2, nu, 250.0, seg, edges, True)
    f32 = ref["frequency"].astype(np.float32)                               # stands in for the device's plane
    index = sm.index32(f32, w, rows, floor2, edges, True)
    differ = index != ref["index"]
    assert not np.any(differ & ~ref["undecidable"]) and ref["undecidable"].mean() < 0.01
    # an entry on an edge goes to the cell above; one on the last edge is out; NaN is out
    planted = np.array([edges[0], edges[3], np.nextafter(edges[3], np.float32(0)), edges[-1], np.nextafter(edges[-1], np.float32(0)),
                        np.nextafter(edges[0], np.float32(0)), np.nan], np.float32)
    inside = np.ones(planted.shape, bool)
    assert sm.cells_of(planted, inside, edges, False).tolist() == [0, 3, 2, -1, 10, -1, -1]
    assert sm.cells_of(planted, inside, edges, True).tolist() == [10, 7, 8, -1, 0, -1, -1]
    assert sm.cells_of(planted, ~inside, edges, False).tolist() == [-1] * 7
    # the chain: bit for bit bandpass's where one cell holds everything; within bandpass's bound of the float64 sums elsewhere
    from bandpass_model import analytic_bound, chains32
    everything = np.zeros((3, 7, 300), np.int32)
    got = sm.chain32(w, rows, g, everything, 1)
    band = chains32(w, [rows], g, np.zeros(9, np.float32))
    assert np.array_equal(got["coefficients"].view(np.uint32), band["analytic"].view(np.uint32))
    got = sm.chain32(w, rows, g, index, 11)
    exact = sm.sums64(w, rows, g, index, 11)
    total = np.tensordot(np.abs(g[1:8]).astype(np.float64), np.abs(w[:, 1:8]).astype(np.float64), axes=(0, 1))   # C, n
    assert np.all(np.abs(got["coefficients"] - exact) <= analytic_bound(7) * total[:, None, :])
    empty = np.broadcast_to((index.max(axis=1) < 0)[:, None, :], got["coefficients"].shape)   # columns with every entry out
    assert got["power"].dtype == np.float32 and np.any(empty) and not np.any(got["coefficients"][empty])
    none = sm.chain32(w, rows, g, np.full((3, 7, 300), -1, np.int32), 11)
    assert not np.any(none["coefficients"]) and not np.any(none["power"])


# -- the condition of the end-to-end test, on the oracle alone -------------------------------------------------------------
@pytest.mark.parametrize("kind,stride", [("morse", 1), ("morse", 4), ("morlet", 1), ("morlet", 4)])
def test_the_chirp_is_decidable_and_sharp_on_the_oracle(kind, stride):
    """What tests/test_gpu_squeeze.py's end-to-end test rests on: with 38 cells and min_amplitude = 0.04 at most 2 % of the
    entries above the threshold are ones whose cell the float64 model cannot decide (frequency within its bound -- rounding,
    the arctangent and the transform's gate -- of an edge, or modulus within the gate of the threshold); and the squeezed
    power is sharper than the rows'."""
    case = sm.chirp_case(kind, stride)
    m = case["model"]
    above = m["above"]
    share = float((above & ~m["decidable"]).sum() / above.sum())
    n = case["n"]
    mid = slice(1500 // stride, n - 1500 // stride)
    inst = sm.chirp_frequency(case["x"].shape[1], stride)
    cells = sm.concentration(m["power"][0], case["centres"], inst, mid)
    one = sm.concentration(m["power"][0], case["centres"], inst, mid, reach=0)
    rows = sm.concentration(case["h"][:, None] * np.abs(case["ref_w"][0]) ** 2, case["f"], inst, mid)
    print("%s, stride %d: %.2f %% of the %d entries above the threshold are undecidable; power in the true cell %.4f, +-1 "
          "%.4f; in the true row +-1 %.4f" % (kind, stride, 100 * share, above.sum(), one, cells, rows))
    assert share <= sm.UNDECIDABLE_CAP
    assert cells > rows and cells >= 0.99
    assert above.mean() > 0.2                                                 # the threshold leaves a band around the sweep
    # the squeezed frequency of what is kept is the sweep's
    kept = (m["index"][0] >= 0)[:, mid]
    f = m["frequency"][0][:, mid]
    assert np.all(np.abs(f[kept] / np.broadcast_to(inst[mid], f.shape)[kept] - 1) < 0.05)


# -- the class and the engine: refusals that need no device ------------------------------------------------------------------
def test_squeeze_before_any_transform_raises():
    from ghost_amd.wave import ContinuousWaveletTransform
    with pytest.raises(ValueError, match="transform"):
        ContinuousWaveletTransform().squeeze()
    with pytest.raises(TypeError):
        ContinuousWaveletTransform().squeeze(38, (20.0, 100.0))               # keywords only


def test_engine_squeeze_refuses_what_it_cannot_use():
    from ghost_amd import engine
    from ghost_amd.multi import ShardedResult
    g, fl, nu, seg = np.ones(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32), np.array([[0, 40], [40, 100]])
    edges = np.array([1.0, 2.0, 4.0], np.float32)
    with pytest.raises(ValueError, match="one device"):
        engine.squeeze(ShardedResult([], (4, 3, 100), True), (0, 3), g, fl, nu, 1000.0, seg, edges)
    with pytest.raises(ValueError, match="complex"):
        engine.squeeze(engine.DeviceResult(object(), (4, 3, 100), 128, False), (0, 3), g, fl, nu, 1000.0, seg, edges)
    with pytest.raises(ValueError, match="freed"):
        engine.squeeze(engine.DeviceResult(None, (4, 3, 100), 128, True), (0, 3), g, fl, nu, 1000.0, seg, edges)
    stub = engine.DeviceResult(object(), (4, 3, 100), 128, True)
    for bad in ((), ("phase",), ("index", "index"), None, 3, ("power", 3), "", ("analytic",)):
        with pytest.raises(ValueError, match="outputs"):
            engine.squeeze(stub, (0, 3), g, fl, nu, 1000.0, seg, edges, False, bad)
    for bad in ((0, 0), (-1, 2), (2, 2), (0, 4), (0.0, 3.0), (True, True), 3, None, (0, 1, 2)):
        with pytest.raises(ValueError, match="rows"):
            engine.squeeze(stub, bad, g, fl, nu, 1000.0, seg, edges)
    for bad in (np.ones(2, np.float32), np.ones((3, 1)), None, np.array([1.0, np.nan, 1.0]), np.array([1.0, np.inf, 1.0]),
                np.ones(3, bool), np.ones(3, complex)):
        with pytest.raises(ValueError, match="'g'"):
            engine.squeeze(stub, (0, 3), bad, fl, nu, 1000.0, seg, edges)
        with pytest.raises(ValueError, match="'floor2'"):
            engine.squeeze(stub, (0, 3), g, bad, nu, 1000.0, seg, edges)
        with pytest.raises(ValueError, match="'nu'"):
            engine.squeeze(stub, (0, 3), g, fl, bad, 1000.0, seg, edges)
    with pytest.raises(ValueError, match="'floor2'.*at least 0"):
        engine.squeeze(stub, (0, 3), g, np.array([0.0, -1.0, 0.0]), nu, 1000.0, seg, edges)
    with pytest.raises(ValueError, match="'nu'.*at least 0"):
        engine.squeeze(stub, (0, 3), g, fl, np.array([0.0, -1.0, 0.0]), 1000.0, seg, edges)
    for bad in (0.0, -1.0, np.nan, np.inf, 1e60, None, "1000", True):
        with pytest.raises(ValueError, match="hz_per_cycle"):
            engine.squeeze(stub, (0, 3), g, fl, nu, bad, seg, edges)
    for bad in ([], [0, 100], [[0, 50, 100]], [[0.0, 100.0]], None):
        with pytest.raises(ValueError, match="'segments'"):
            engine.squeeze(stub, (0, 3), g, fl, nu, 1000.0, np.array(bad) if bad is not None else None, edges)
    with pytest.raises(ValueError, match=r"segments\[1\]"):
        engine.squeeze(stub, (0, 3), g, fl, nu, 1000.0, np.array([[0, 40], [41, 100]]), edges)
    for bad in ([], [1.0], [[1.0, 2.0]], None, np.array([True, True]), np.array([1.0, 2.0], complex), [0.0, 1.0], [-1.0, 1.0],
                [1.0, np.nan], [1.0, np.inf], [1.0, 1e60], [1.0, 1.0], [2.0, 1.0], [1.0, 1.0 + 1e-9], np.arange(1.0, 4099.0)):
        with pytest.raises(ValueError, match="'edges'"):
            engine.squeeze(stub, (0, 3), g, fl, nu, 1000.0, seg, bad)
    with pytest.raises(ValueError, match=r"edges\[2\]"):
        engine.squeeze(stub, (0, 3), g, fl, nu, 1000.0, seg, [1.0, 2.0, 2.0, 3.0])
    for bad in (None, 1, "yes"):
        with pytest.raises(ValueError, match="descending"):
            engine.squeeze(stub, (0, 3), g, fl, nu, 1000.0, seg, edges, bad)


def test_class_squeeze_refuses_results_and_arguments_it_cannot_use():
    from ghost_amd import engine
    from ghost_amd.multi import ShardedResult
    from ghost_amd.wave import ContinuousWaveletTransform
    cwt = ContinuousWaveletTransform()
    cwt._frequencies, cwt._fs = np.geomspace(100.0, 10.0, 3), FS
    cwt._device_result, cwt._pending = engine.DeviceResult(object(), (1, 3, 100), 128, False), ("amplitude", np.float32, True)
    with pytest.raises(ValueError, match="output='complex'"):
        cwt.squeeze()
    cwt._device_result, cwt._pending = ShardedResult([], (4, 3, 100), True), ("complex", np.float32, False)
    with pytest.raises(ValueError, match="sharded"):
        cwt.squeeze()
    cwt._device_result = engine.DeviceResult(object(), (1, 3, 100), 128, True)
    with pytest.raises(ValueError, match="freq_limits"):
        cwt.squeeze(freq_limits=(200.0, 300.0))
    with pytest.raises(ValueError, match="at least 2 selected rows"):
        cwt.squeeze(freq_limits=(90.0, 110.0))
    with pytest.raises(ValueError, match="at least 2 selected rows"):
        cwt.squeeze(5, freq_limits=(90.0, 110.0))
    for bad in (1, 0, -3, True, "38", [[1.0, 2.0]], 2.5):
        with pytest.raises(ValueError, match="'bins'"):
            cwt.squeeze(bad)
    with pytest.raises(ValueError, match="monotonic"):
        cwt.squeeze([10.0, 30.0, 20.0])
    with pytest.raises(ValueError, match="at least 2"):
        cwt.squeeze([10.0])
    for bad in (-1.0, np.nan, np.inf, None, "0.1", True):
        with pytest.raises(ValueError, match="min_amplitude"):
            cwt.squeeze(min_amplitude=bad)
    with pytest.raises(ValueError, match="min_amplitude"):
        cwt.squeeze(min_amplitude=1e30)
    with pytest.raises(ValueError, match="outputs"):
        cwt.squeeze(outputs=("analytic",))
    cwt._device_result = engine.DeviceResult(None, (1, 3, 100), 128, True)
    with pytest.raises(ValueError, match="freed"):
        cwt.squeeze()
    cwt._device_result = None


def test_bins_none_takes_the_rows_own_frequencies_on_a_descending_grid(monkeypatch):
    """The default grid descends: the cells are the rows' own, ``bin_frequencies`` keeps the rows' order, the edges ascend,
    and the engine is told that output row k is cell L - 1 - k.  The engine call itself is replaced: no device is needed for
    what the class prepares."""
    from ghost_amd import engine
    from ghost_amd.wave import ContinuousWaveletTransform
    from ghost_amd.wave.morse import Morse
    f = np.geomspace(120.0, 15.0, 13)
    cwt = ContinuousWaveletTransform(wavelet=Morse(fs=FS, gamma=3.0, beta=20.0))
    cwt._frequencies, cwt._fs, cwt._stride = f, FS, 4
    cwt._device_result, cwt._pending = engine.DeviceResult(object(), (1, 13, 100), 128, True), ("complex", np.float32, True)
    seen = {}

    class Stub:
        def to_host(self):
            return {"index": np.zeros((1, seen["rows"][1], 100), np.int32)}

        def free(self):
            seen["freed"] = True

    def fake(result, rows, g, floor2, nu, hz, segments, edges, descending, outputs):
        seen.update(rows=rows, g=g, floor2=floor2, nu=nu, hz=hz, segments=segments, edges=edges, descending=descending, outputs=outputs)
        return Stub()

    monkeypatch.setattr(engine, "squeeze", fake)
    monkeypatch.setattr(type(cwt), "time", property(lambda self: None))
    got = cwt.squeeze(freq_limits=(20.0, 100.0), min_amplitude=0.5, outputs=("index",))
    rows = engine.coupling_rows((20.0, 100.0), f, "freq_limits")
    own = f[rows[0]:rows[0] + rows[1]]
    assert seen["rows"] == rows and seen["descending"] is True and seen["outputs"] == ("index",) and seen["freed"]
    assert np.array_equal(got.bin_frequencies, own) and np.array_equal(got.frequencies, own) and got.rows == rows
    want, desc = engine.squeeze_edges(own)
    assert desc and np.array_equal(seen["edges"], want) and np.array_equal(got.edges, want) and np.all(np.diff(got.edges) > 0)
    assert np.all(got.edges[:-1] < own[::-1]) and np.all(own[::-1] < got.edges[1:])
    assert np.array_equal(seen["g"], engine.band_weights(f, cwt._wavelet)[0])
    assert seen["floor2"].dtype == np.float32 and np.array_equal(seen["floor2"], np.full(13, 0.25, np.float32))   # Morse: e = 1
    assert np.allclose(seen["nu"], 2 * np.pi * f * 4 / FS) and seen["hz"] == FS / 4
    assert np.array_equal(seen["segments"], [[0, 100]])
    assert got.index.shape == (rows[1], 100) and got.coefficients is None and got.power is None and got.frequency is None
    assert got.min_amplitude == 0.5 and got.time is None
    # an int: geomspace between the selected rows' end frequencies, in the rows' order; an array: as given
    got = cwt.squeeze(7, freq_limits=(20.0, 100.0), outputs=("index",))
    assert np.allclose(got.bin_frequencies, np.geomspace(own[0], own[-1], 7)) and seen["descending"] is True and seen["edges"].size == 8
    got = cwt.squeeze([30.0, 40.0, 55.0], outputs=("index",))
    assert np.array_equal(got.bin_frequencies, [30.0, 40.0, 55.0]) and seen["descending"] is False and seen["rows"] == (0, 13)
    cwt._device_result = None


# -- the C entry point: arguments first, then the device --------------------------------------------------------------------
def test_entry_point_validates_then_needs_a_device():
    from ghost_amd import _lib
    from ghost_amd.engine import device_count
    lib = _lib.lib
    assert (_lib.SQUEEZE_TILE_COLS, _lib.SQUEEZE_GROUP_CELLS, _lib.SQUEEZE_MAX_CELLS) == (512, 16, 4096)
    buf = (C.c_float * 512)()
    any4 = (C.c_float * 4)(1.0, -2.0, 0.0, 3.0)
    fl4 = (C.c_float * 4)(0.0, 2.0, 0.5, 3.0)
    adv = (C.c_float * 4)(0.0, 2.0, 0.5, 9.0)
    two = (C.c_int64 * 4)(0, 7, 7, 16)
    ed3 = (C.c_float * 4)(1.0, 2.0, 4.0, 8.0)
    many = (C.c_float * 4098)(*np.arange(1.0, 4099.0))

    def call(rows=buf, pitch=16, c=1, s=4, n=16, first=1, count=3, g=any4, fl=fl4, nu=adv, hz=1000.0, seg=two, n_seg=2, edges=ed3,
             n_cells=3, desc=0, coef=buf, pw=buf, frq=buf, idx=buf, out_pitch=16):
        return lib.gcwt_squeeze(rows, pitch, c, s, n, first, count, g, fl, nu, hz, seg, n_seg, edges, n_cells, desc, coef, pw, frq,
                                C.cast(idx, C.c_void_p) if idx is not None else None, out_pitch)

    def f4(*v):
        return (C.c_float * 4)(*v)

    def s4(*v):
        return (C.c_int64 * 4)(*v)

    for kw, word in ((dict(rows=None), b"d_rows is NULL"), (dict(g=None), b"g is NULL"), (dict(fl=None), b"floor2 is NULL"),
                     (dict(nu=None), b"nu is NULL"), (dict(seg=None), b"segments"), (dict(n_seg=0), b"segments"),
                     (dict(edges=None), b"edges is NULL"), (dict(c=0), b"n_channels"), (dict(s=0), b"n_scales"), (dict(n=0), b"n_cols"),
                     (dict(pitch=15), b"pitch"), (dict(first=-1), b"rows"), (dict(count=0), b"rows"), (dict(first=2, count=3), b"rows"),
                     (dict(g=f4(1, float("nan"), 1, 1)), b"g[1]"), (dict(g=f4(1, 1, 1, float("inf"))), b"g[3]"),
                     (dict(fl=f4(0, float("nan"), 1, 1)), b"floor2[1]"), (dict(fl=f4(0, 1, -1e-30, 1)), b"floor2[2]"),
                     (dict(fl=f4(float("inf"), 1, 1, 1)), b"floor2[0]"),
                     (dict(nu=f4(0, float("nan"), 1, 1)), b"nu[1]"), (dict(nu=f4(0, 1, -1e-30, 1)), b"nu[2]"),
                     (dict(nu=f4(0, 1, 1, float("inf"))), b"nu[3]"), (dict(hz=0.0), b"hz_per_cycle"),
                     (dict(hz=float("nan")), b"hz_per_cycle"), (dict(hz=-1.0), b"hz_per_cycle"),
                     (dict(seg=s4(0, 0, 0, 16)), b"segments[0]"), (dict(seg=s4(1, 7, 7, 16)), b"segments[0]"),
                     (dict(seg=s4(0, 7, 8, 16)), b"segments[1]"), (dict(seg=s4(0, 7, 6, 16)), b"segments[1]"),
                     (dict(seg=s4(0, 7, 7, 17)), b"segments[1]"), (dict(seg=s4(0, 7, 7, 15)), b"segments[1]"),
                     (dict(n_seg=1), b"segments[0]"), (dict(n_seg=17), b"segments"),
                     (dict(n_cells=0), b"n_cells"), (dict(n_cells=4097, edges=many), b"n_cells"),
                     (dict(edges=f4(0, 1, 2, 3)), b"edges[0]"), (dict(edges=f4(1, float("nan"), 2, 3)), b"edges[1]"),
                     (dict(edges=f4(1, 2, 3, float("inf"))), b"edges[3]"), (dict(edges=f4(-1, 2, 3, 4)), b"edges[0]"),
                     (dict(edges=f4(1, 2, 2, 3)), b"edges[2]"), (dict(edges=f4(1, 3, 2, 4)), b"edges[2]"),
                     (dict(edges=f4(1, 2, 3, 3)), b"strictly ascending"),
                     (dict(out_pitch=15), b"out_pitch"), (dict(coef=None, pw=None, frq=None, idx=None), b"nothing"),
                     (dict(c=2**31 - 1, n=2**40, pitch=2**40, out_pitch=2**40, seg=s4(0, 7, 7, 2**40)), b"workgroups")):
        assert call(**kw) == _lib.ERR_INVALID, kw
        msg = lib.gcwt_last_error()
        assert msg.startswith(b"gcwt_squeeze:") and word in msg, (kw, msg)
    # a valid request: without a GPU there is nothing that computes it; with one, host memory is not a resident result
    n_dev = device_count()
    for kw in (dict(), dict(frq=None, idx=None), dict(coef=None, pw=None), dict(n_cells=1), dict(n_cells=2, edges=f4(1, 2, 3, 3)),
               dict(seg=s4(0, 16, 0, 0), n_seg=1), dict(n=15, seg=s4(0, 1, 1, 15)), dict(desc=1), dict(first=0, count=4),
               dict(n_cells=4096, edges=many), dict(g=f4(0, 0, 0, 0), fl=f4(0, 0, 0, 0), nu=f4(0, 0, 0, 0))):
        rc = call(**kw)
        if n_dev == 0:
            assert rc == _lib.ERR_NO_DEVICE and b"no CPU path" in lib.gcwt_last_error(), kw
        else:
            assert rc == _lib.ERR_INVALID and b"device memory" in lib.gcwt_last_error(), kw
