"""coherence() on the host side (no GPU): the pair validator, the argument checks of gcwt_coherence before any device
call, the tiling of a pair list into tasks (include/ghostcwt_debug.h: gcwt_debug_coherence_tasks), and the float64
model of the definition (tests/coherence_model.py) on the oracle's coefficients."""
import ctypes as C

import numpy as np
import pytest

import coherence_model as cm
from oracle import ghost_oracle as orc


# -- the validator ----------------------------------------------------------------------------------------------------
def test_default_is_all_pairs_in_lexicographic_order():
    from ghost_amd.engine import coherence_pairs
    p = coherence_pairs(None, None, 4)
    assert p.dtype == np.int32 and p.tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    np.testing.assert_array_equal(coherence_pairs(None, None, 17), cm.all_pairs(17))
    assert coherence_pairs(None, None, 2).tolist() == [[0, 1]]


def test_seed_is_the_seed_against_every_other_channel_ascending():
    from ghost_amd.engine import coherence_pairs
    assert coherence_pairs(None, 2, 5).tolist() == [[2, 0], [2, 1], [2, 3], [2, 4]]
    assert coherence_pairs(None, 0, 3).tolist() == [[0, 1], [0, 2]]
    assert coherence_pairs(None, np.int64(4), 5).tolist() == [[4, 0], [4, 1], [4, 2], [4, 3]]
    np.testing.assert_array_equal(coherence_pairs(None, 9, 17), cm.seed_pairs(9, 17))


@pytest.mark.parametrize("pairs", [[[0, 1]], [[3, 0], [0, 3], [0, 3]], np.array([[1, 2], [2, 1]], dtype=np.uint8),
                                   np.array([[0, 4]], dtype=np.int64), ((1, 0), (2, 0))])
def test_explicit_pairs_are_kept_as_given(pairs):
    from ghost_amd.engine import coherence_pairs
    p = coherence_pairs(pairs, None, 5)
    assert p.dtype == np.int32 and p.flags.c_contiguous
    np.testing.assert_array_equal(p, np.asarray(pairs))


@pytest.mark.parametrize("pairs,seed,n", [
    ([[0.0, 1.0]], None, 4), ([[True, False]], None, 4), ([[1, 1]], None, 4), ([[0, 4]], None, 4), ([[-1, 2]], None, 4),
    ([[0, 1]], 0, 4), ([0, 1], None, 4), ([[0, 1, 2]], None, 4), (np.zeros((0, 2), np.int64), None, 4), ("01", None, 4),
    (None, 4, 4), (None, -1, 4), (None, 1.0, 4), (None, True, 4), (None, "1", 4), (None, None, 1), (None, 0, 1),
    ([[0, 1]], None, 1), ([[0, 1], [2, 2]], None, 4)])
def test_validator_refuses(pairs, seed, n):
    from ghost_amd.engine import coherence_pairs
    with pytest.raises(ValueError):
        coherence_pairs(pairs, seed, n)


@pytest.mark.parametrize("bad", [1, 0, -5, 2.0, 64.5, True, "64", None])
def test_window_must_be_an_integer_of_at_least_two(bad):
    from ghost_amd.engine import coherence_window
    with pytest.raises(ValueError, match="window"):
        coherence_window(bad)
    assert coherence_window(2) == 2 and coherence_window(np.int32(1000)) == 1000


def test_coherence_before_any_transform_raises():
    from ghost_amd.wave import ContinuousWaveletTransform
    with pytest.raises(ValueError, match="transform"):
        ContinuousWaveletTransform().coherence(window=64)
    with pytest.raises(ValueError, match="window"):
        ContinuousWaveletTransform().coherence(window=1)
    with pytest.raises(TypeError):
        ContinuousWaveletTransform().coherence()               # window is required


def test_engine_coherence_refuses_what_is_not_a_complex_device_result():
    from ghost_amd import engine
    from ghost_amd.multi import ShardedResult
    with pytest.raises(ValueError, match="one device"):
        engine.coherence(ShardedResult([], (4, 3, 100), True), None, 64)
    with pytest.raises(ValueError, match="complex"):
        engine.coherence(engine.DeviceResult(object(), (4, 3, 100), 128, False), None, 64)
    with pytest.raises(ValueError, match="window"):
        engine.coherence(engine.DeviceResult(object(), (4, 3, 100), 128, True), None, 1)


# -- the C entry point: arguments first, then the device ----------------------------------------------------------------
def test_entry_point_validates_then_needs_a_device():
    from ghost_amd import _lib
    from ghost_amd.engine import device_count
    lib = _lib.lib
    buf = (C.c_float * 64)()
    i32p = C.POINTER(C.c_int32)

    def call(rows=buf, pitch=16, c=3, s=1, n=16, pairs=((0, 1),), window=4, power=buf, cross=buf, coh=buf, out_pitch=4):
        arr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        return lib.gcwt_coherence(rows, pitch, c, s, n, arr.ctypes.data_as(i32p) if arr.size else None, len(arr),
                                  window, power, cross, coh, out_pitch)

    for kw, word in ((dict(rows=None), b"NULL"), (dict(window=1), b"window"), (dict(window=0), b"window"),
                     (dict(pitch=15), b"pitch"), (dict(n=0), b"n_cols"), (dict(s=0), b"n_scales"),
                     (dict(c=0), b"n_channels"), (dict(pairs=((0, 3),)), b"outside"), (dict(pairs=((-1, 1),)), b"outside"),
                     (dict(pairs=((2, 2),)), b"itself"), (dict(out_pitch=3), b"out_pitch"),
                     (dict(power=None, cross=None, coh=None), b"nothing"), (dict(pairs=(), power=None), b"nothing")):
        assert call(**kw) == _lib.ERR_INVALID, kw
        assert word in lib.gcwt_last_error(), (kw, lib.gcwt_last_error())
    assert lib.gcwt_coherence(buf, 16, 3, 1, 16, None, 1, 4, buf, buf, buf, 4) == _lib.ERR_INVALID   # pairs NULL, n_pairs 1
    # a valid request: without a GPU there is nothing that computes it; with one, host memory is not a resident result
    n_dev = device_count()
    rc = call()
    if n_dev == 0:
        assert rc == _lib.ERR_NO_DEVICE and b"no CPU path" in lib.gcwt_last_error()
    else:
        assert rc == _lib.ERR_INVALID and b"device memory" in lib.gcwt_last_error()


# -- the tiling ------------------------------------------------------------------------------------------------------------
def _tasks(n_channels, pairs):
    from ghost_amd import _lib
    lib = _lib.lib
    i32p = C.POINTER(C.c_int32)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    pp = pairs.ctypes.data_as(i32p) if pairs.size else None
    n = lib.gcwt_debug_coherence_tasks(n_channels, pp, len(pairs), None, None, None, None, None, 0)
    assert n >= 0, lib.gcwt_last_error()
    ta, tb, fl = (np.zeros(n, np.int32) for _ in range(3))
    first = np.zeros(n + 1, np.int32)
    ent = np.zeros((max(1, len(pairs)), 3), np.int32)
    assert lib.gcwt_debug_coherence_tasks(n_channels, pp, len(pairs), ta.ctypes.data_as(i32p), tb.ctypes.data_as(i32p),
                                          fl.ctypes.data_as(i32p), first.ctypes.data_as(i32p), ent.ctypes.data_as(i32p), n) == n
    return [{"a": int(ta[i]), "b": int(tb[i]), "flags": int(fl[i]), "entries": ent[first[i]:first[i + 1]].tolist()}
            for i in range(n)]


def _check_tiling(n_channels, pairs):
    from ghost_amd import _lib
    lib = _lib.lib
    assert lib.gcwt_debug_coherence_tasks(1, None, 0, None, None, None, None, None, 0) == 1
    T = 8
    pairs = np.asarray(pairs).reshape(-1, 2)
    tasks = _tasks(n_channels, pairs)
    n_tiles = -(-n_channels // T)
    seen_rows, seen_tiles, power = [], set(), []
    emptied = False
    for t in tasks:
        assert 0 <= t["a"] <= t["b"] < n_tiles
        if not t["entries"]:                      # power alone: a tile no pair touches, after every task with entries
            emptied = True
            assert t["a"] == t["b"] and t["flags"] == 1
        else:
            assert not emptied
            assert (t["a"], t["b"]) not in seen_tiles, "a tile pair twice"
            seen_tiles.add((t["a"], t["b"]))
        if t["a"] == t["b"]:
            assert t["flags"] in (0, 1)
        power += [t["a"]] * (t["flags"] & 1) + [t["b"]] * ((t["flags"] >> 1) & 1)
        for cell, conj, row in t["entries"]:
            i, j = divmod(cell, T)
            ca, cb = t["a"] * T + i, t["b"] * T + j
            assert ca < n_channels and cb < n_channels and ca < cb
            want = (cb, ca) if conj else (ca, cb)
            assert tuple(pairs[row]) == want, (t, cell, conj, row)
            seen_rows.append(row)
    assert sorted(seen_rows) == list(range(len(pairs))), "every wanted pair in exactly one task"
    assert sorted(power) == list(range(n_tiles)), "every tile's power written by exactly one task"
    return tasks


def test_tiling_all_pairs_of_17_channels_with_a_ragged_last_tile():
    tasks = _check_tiling(17, cm.all_pairs(17))
    assert [(t["a"], t["b"]) for t in tasks] == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2)]   # tile 2 holds one channel
    assert [len(t["entries"]) for t in tasks] == [28, 64, 8, 28, 8]
    assert len(_check_tiling(128, cm.all_pairs(128))) == 136


def test_tiling_a_seed():
    tasks = _check_tiling(17, cm.seed_pairs(9, 17))
    assert [(t["a"], t["b"]) for t in tasks] == [(0, 1), (1, 1), (1, 2)]
    # seed 9 paired with lower channels is the conjugated cell
    conj = {tuple(cm.seed_pairs(9, 17)[row]): c for t in tasks for _, c, row in t["entries"]}
    assert all(c == (k < 9) for (_, k), c in conj.items())
    assert len(_check_tiling(128, cm.seed_pairs(0, 128))) == 16


def test_tiling_a_list_with_repeats_and_both_orders():
    pairs = [[3, 12], [12, 3], [3, 12], [1, 2], [2, 1], [16, 0], [0, 16], [5, 4]]
    tasks = _check_tiling(17, pairs)
    assert [(t["a"], t["b"]) for t in tasks] == [(0, 0), (0, 1), (0, 2)]
    cells = {}
    for t in tasks:
        for cell, conj, row in t["entries"]:
            cells.setdefault((t["a"], t["b"], cell), []).append((row, conj))
    assert sorted(cells[(0, 1, 3 * 8 + 4)]) == [(0, 0), (1, 1), (2, 0)]      # one cell, three output rows
    assert sorted(cells[(0, 0, 1 * 8 + 2)]) == [(3, 0), (4, 1)]
    assert sorted(cells[(0, 2, 0)]) == [(5, 1), (6, 0)]


def test_tiling_gives_untouched_tiles_a_power_task():
    tasks = _check_tiling(40, [[0, 1], [33, 2]])
    assert [(t["a"], t["b"], t["flags"], len(t["entries"])) for t in tasks] == \
        [(0, 0, 1, 1), (0, 4, 2, 1), (1, 1, 1, 0), (2, 2, 1, 0), (3, 3, 1, 0)]


# -- the model on the oracle ---------------------------------------------------------------------------------------------
def test_model_sums_are_the_definition():
    rng = np.random.default_rng(3)
    w = rng.standard_normal((3, 2, 23)) + 1j * rng.standard_normal((3, 2, 23))
    w[2, :, 10:20] = 0
    m = cm.model(w, [[0, 1], [2, 0]], 5)
    assert m["cross"].shape == (2, 2, 5) and m["power"].shape == (3, 2, 5) and m["counts"].tolist() == [5, 5, 5, 5, 3]
    np.testing.assert_allclose(m["cross"][1, 1, 4], np.mean(w[2, 1, 20:23] * np.conj(w[0, 1, 20:23])), rtol=1e-14)
    np.testing.assert_allclose(m["power"][1, 0, 2], np.mean(np.abs(w[1, 0, 10:15]) ** 2), rtol=1e-14)
    assert np.all(m["coherence"][1, :, 2:4] == 0) and np.all(m["cross"][1, :, 2:4] == 0) and np.all(m["power"][2, :, 2:4] == 0)
    assert m["coherence"].min() >= 0 and m["coherence"].max() <= 1 + 1e-12
    one = cm.model(np.stack([w[0], 2j * w[0]]), [[0, 1]], 4)             # a channel with its own multiple
    np.testing.assert_allclose(one["coherence"], 1.0, rtol=1e-12)
    np.testing.assert_allclose(np.angle(one["cross"]), -np.pi / 2, rtol=1e-12)


def test_model_on_the_oracle_finds_the_locked_pair_its_lag_and_the_unrelated_channel():
    n, fs = 32768, 1000.0
    x = cm.three_channel_input(n, fs)
    f = orc.frequency_grid(fs, n, freq_limits=(2, 300), voices_per_octave=4)
    rows = [int(np.argmin(np.abs(f - 8.0))), int(np.argmin(np.abs(f - 100.0)))]
    w = np.stack([orc.cwt_complex(x[c], fs, f[rows]) for c in range(3)])
    m = cm.model(w, [[0, 1], [0, 2]], 256)
    coh01 = float(np.median(m["coherence"][0, 0]))
    lag01 = float(np.median(np.angle(m["cross"][0, 0])))
    coh02 = float(np.median(m["coherence"][1, 1]))
    print("coherence (0,1) at 8 Hz %.4f, angle %.4f rad, coherence (0,2) at 100 Hz %.4f" % (coh01, lag01, coh02))
    assert coh01 >= 0.99
    assert abs(lag01 - 0.7) <= 0.02
    assert coh02 <= 0.2
