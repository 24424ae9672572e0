"""output_stride on the host side (no GPU): argument checks before any device work, the C setter, and the output
sizes a plan reports (include/ghostcwt.h: gcwt_plan_set_output_stride)."""
import ctypes as C

import numpy as np
import pytest


@pytest.mark.parametrize("bad", [0, -3, 2.5, True, np.bool_(True), "4", 2.0])
def test_transform_rejects_a_bad_stride_before_any_device_work(bad, monkeypatch):
    from ghost_amd import engine
    from ghost_amd.wave import ContinuousWaveletTransform

    def no_plan(*a, **k):
        raise AssertionError("a plan was made for a bad output_stride")
    monkeypatch.setattr(engine, "CwtPlan", no_plan)
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    with pytest.raises(ValueError, match="output_stride"):
        ContinuousWaveletTransform().transform(x, fs=1000.0, freq_limits=[10, 100], output_stride=bad)


def test_numpy_integers_are_strides():
    from ghost_amd.engine import output_stride_value
    assert output_stride_value(np.int64(30)) == 30 and output_stride_value(np.uint8(2)) == 2
    assert output_stride_value(1) == 1


def _host_plan(n, k=1, c=3, output="amplitude"):
    from ghost_amd.engine import CwtPlan
    return CwtPlan(n, c, 1000.0, np.array([120.0, 40.0, 9.0, 3.0]), output=output, output_stride=k)


def test_setter_refuses_a_stride_below_one():
    from ghost_amd import _lib
    p = _host_plan(5000)
    assert _lib.lib.gcwt_plan_set_output_stride(p._handle, 0) == _lib.ERR_INVALID
    assert _lib.lib.gcwt_plan_set_output_stride(p._handle, -7) == _lib.ERR_INVALID
    assert _lib.lib.gcwt_plan_set_output_stride(p._handle, 4) == 0
    with pytest.raises(ValueError):
        _host_plan(5000, k=0)


@pytest.mark.parametrize("n,k", [(5000, 1), (5000, 2), (5000, 3), (5001, 7), (4096, 256), (999, 1000), (30000, 30)])
@pytest.mark.parametrize("output", ["amplitude", "complex"])
def test_out_bytes_count_the_kept_columns(n, k, output):
    p = _host_plan(n, k, output=output)
    cols = -(-n // k)
    elem = 8 if output == "complex" else 4
    assert p.info["out_bytes"] == 3 * 4 * cols * elem
    assert p.out_shape == (3, 4, cols)


def _stride_keep(n, k):
    """kernels.h: stride_keep in 32-bit arithmetic, for recording samples n (uint64, below 2^31): q = umulhi(n,
    ceil(2^32 / K)) and whether q K == n (mod 2^32)."""
    magic = np.uint64(((1 << 32) + int(k) - 1) // int(k))
    q = (n * magic) >> np.uint64(32)
    return ((q * np.uint64(k)) & np.uint64(0xFFFFFFFF)) == n, q


LARGE_STRIDES = [4097, 5000, 65535, 65536, 65537, 99991, (1 << 17) + 1, 1000003, (1 << 20) - 1, 1 << 20]


@pytest.mark.parametrize("ks", [range(2, 1025), range(1025, 4097), LARGE_STRIDES], ids=["2-1024", "1025-4096", "large"])
def test_multiply_high_finds_the_column_of_every_multiple(ks):
    """umulhi(n, ceil(2^32 / K)) == n // K for the multiples n of K below 2^31: the first and the last 512 of them and
    1024 spread over the range (the product's error term n e / K, e < K, grows with n: the top is the tight end)."""
    top = (1 << 31) - 1
    for k in ks:
        last = top // k
        j = np.unique(np.concatenate([np.arange(0, min(512, last + 1)), np.arange(max(0, last - 511), last + 1),
                                      np.linspace(0, last, 1024).astype(np.int64)])).astype(np.uint64)
        n = j * np.uint64(k)
        assert int(n.max()) <= top
        kept, q = _stride_keep(n, k)
        assert kept.all(), (k, n[~kept][:4])
        np.testing.assert_array_equal(q, j, err_msg="K=%d" % k)


@pytest.mark.parametrize("ks", [range(2, 1025), range(1025, 4097), LARGE_STRIDES], ids=["2-1024", "1025-4096", "large"])
def test_multiply_high_rejects_every_other_sample(ks):
    """The keep test (q K == n in 32 bits) holds for the multiples of K alone: every sample of windows of 4096 near 0
    and near 2^31, and of K-sample runs spread in between."""
    top = (1 << 31) - 1
    for k in ks:
        runs = [np.arange(s, s + k) for s in np.linspace(0, top - k, 9).astype(np.int64)]
        n = np.unique(np.concatenate([np.arange(0, 4096), np.arange(top - 4095, top + 1)] + runs)).astype(np.uint64)
        kept, q = _stride_keep(n, k)
        np.testing.assert_array_equal(kept, n % np.uint64(k) == 0, err_msg="K=%d" % k)
        np.testing.assert_array_equal(q[kept], n[kept] // np.uint64(k))


def test_stride_may_change_until_the_plan_runs():
    """A plan created, its stride changed while nothing has run: the plan reports the new size each time."""
    from ghost_amd import _lib
    p = _host_plan(10000)
    for k, cols in ((1, 10000), (3, 3334), (10000, 1), (10001, 1)):
        assert _lib.lib.gcwt_plan_set_output_stride(p._handle, k) == 0
        info = _lib.PlanInfo()
        assert _lib.lib.gcwt_plan_get_info(p._handle, C.byref(info)) == 0
        assert info.out_bytes == 3 * 4 * cols * 4
