"""Options early_interp and interp_split_r (csrc/api.cpp: run_pipeline) on the device (GPU).  With early_interp = 1
the level passes k_synthi reads (group H: the levels an interpolated level takes its x_R from) run on the plan's own
stream with k_synthi right behind them while the other passes (group L) run on the two side streams and are joined in
front of the first kernel that reads them; early_interp = 0 (the default) joins every pass before any synthesis kernel
starts.  k_synthi is two launches cut at interp_split_r (default 64), one with interp_split_r = 0.  Nothing about the
arithmetic differs, so every case here holds a plan with early_interp = 1 bit-equal, in one process, to the same plan in
the joined order with one launch, and one of the two to the oracle at the project's gate, 1e-5 of the row's peak
(conftest.rel_err), power included.

The grid is six voices per octave from 200 Hz down to 2 Hz at 1 kHz: decimations 2, 4, 8 (k_synth7: group L) and 16,
32, 64, 128 (k_synthi: group H)."""
import numpy as np
import pytest

import channel_cases as cc
import morlet_cases as mc
from conftest import rel_err
from oracle import ghost_oracle as orc

pytestmark = pytest.mark.gpu

FS = cc.FS
TOL = 1e-5
F6 = 200.0 / 2.0 ** (np.arange(40) / 6.0)
N = 16384
_CACHE = {}


class _Options:
    """Library switches for the plans made inside the ``with`` (they are read when a plan is created)."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from ghost_amd.engine import set_option
        for k, v in self.kw.items():
            set_option(k, v)

    def __exit__(self, *exc):
        from ghost_amd.engine import set_option
        for k in self.kw:
            set_option(k, None)


def _pair(make, early=1, **early_options):
    """(the plan of ``make()`` under early_interp = ``early`` and ``early_options``, the same under early_interp = 0 and
    interp_split_r = 0: every level pass joined first, one k_synthi launch)."""
    with _Options(early_interp=early, **early_options):
        early = make()
    with _Options(early_interp=0, interp_split_r=0):
        joined = make()
    return early, joined


def _groups(plan):
    """(decimations of group H, decimations of group L): a decimation's levels share one x_R."""
    lv, di = plan.debug_levels(), plan.debug_interp()["levels"]
    h = {l["decimation"] for l, d in zip(lv, di) if d is not None}
    return sorted(h), sorted({l["decimation"] for l in lv} - h)


def _plan(n, c, f=F6, **kw):
    from ghost_amd.engine import CwtPlan
    return CwtPlan(n, c, FS, f, **kw)


def _base(n=N):
    if ("base", n) not in _CACHE:
        b = cc.base_signals(n)
        b.setflags(write=False)
        _CACHE[("base", n)] = b
    return _CACHE[("base", n)]


def _oracle(key, make):
    """A reference made once and left as it is."""
    if key not in _CACHE:
        ref = make()
        ref.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]


def _ref_base(f=F6, n=N, **kw):
    """complex128 (5, S, n): the oracle's rows of the five base signals."""
    key = ("ref", n, tuple(np.round(f, 9)), tuple(sorted((k, str(v)) for k, v in kw.items())))
    return _oracle(key, lambda: cc.oracle_base(_base(n), f, "complex", **kw))


def _gate(what, got, ref_base, output):
    err = cc.oracle_error(got, cc.as_output(output, ref_base), output)
    print("    %s: worst row %.3g of the row's peak (gate %.0e)" % (what, err.max(), TOL))
    assert err.max() <= TOL, (what, float(err.max()))


def _both(what, early, joined, x, ref_base, output):
    got, want = early.execute(x), joined.execute(x)
    assert np.array_equal(got, want), what
    _gate(what, got, ref_base, output)
    return got


# ---- output modes, channel counts, the cut between the two launches ---------------------------------------------------
@pytest.mark.parametrize("n_channels", [1, 2, 33])
@pytest.mark.parametrize("output", ["amplitude", "power"])
def test_modes_and_channels(output, n_channels):
    """Amplitude and power, 1, 2 and 33 channels, every one told apart from every other (channel_cases.expand)."""
    early, joined = _pair(lambda: _plan(N, n_channels, output=output))
    assert _groups(early) == ([16, 32, 64, 128], [2, 4, 8])
    x = cc.expand(_base(), n_channels)
    _both("%s, %d channels" % (output, n_channels), early, joined, x, _ref_base(), output)
    early.close(); joined.close()


def test_complex_output_has_no_interpolated_level():
    """Complex rows are all k_synth7's: the plan has no group H and runs in the joined order whatever the option says."""
    early, joined = _pair(lambda: _plan(N, 2, output="complex"))
    assert early.info["n_interp"] == 0 and _groups(early)[0] == []
    _both("complex", early, joined, cc.expand(_base(), 2), _ref_base(), "complex")
    early.close(); joined.close()


@pytest.mark.parametrize("early", [1, 0])
@pytest.mark.parametrize("split_r", [16, 64, 1 << 20])
def test_split_between_the_two_launches(split_r, early):
    """interp_split_r = 16: the first k_synthi launch is empty; 64: the default, R = 16, 32 | 64, 128; 2^20: the second
    one is empty and (early_interp = 1) the side streams' passes overlap all of k_synthi.  Under either order."""
    plan, joined = _pair(lambda: _plan(N, 2), early=early, interp_split_r=split_r)
    _both("early_interp = %d, interp_split_r = %d" % (early, split_r), plan, joined, cc.expand(_base(), 2), _ref_base(),
          "amplitude")
    plan.close(); joined.close()


@pytest.mark.parametrize("output", ["amplitude", "power"])
def test_default_plan(output, option):
    """The plan as it is made with no option set -- two k_synthi launches in the joined order -- on 33 channels."""
    plan = _plan(N, 33, output=output)
    option("early_interp", 0)
    option("interp_split_r", 0)
    joined = _plan(N, 33, output=output)
    _both("default, %s" % output, plan, joined, cc.expand(_base(), 33), _ref_base(), output)
    plan.close(); joined.close()


# ---- degenerate groupings ---------------------------------------------------------------------------------------------
def test_only_interpolated_levels():
    """Every level is in group H: the side streams stay empty, the batch must still end joined."""
    f = F6[F6 < 21.0]
    early, joined = _pair(lambda: _plan(N, 2, f))
    assert _groups(early) == ([16, 32, 64, 128], [])
    x = cc.expand(_base(), 2)
    first = _both("R >= 16 only", early, joined, x, _ref_base(f), "amplitude")
    assert np.array_equal(early.execute(x), first)
    early.close(); joined.close()


def test_no_interpolated_level():
    """Every level is in group L (R <= 8): nothing to start early."""
    f = F6[F6 > 24.0]
    early, joined = _pair(lambda: _plan(N, 2, f))
    assert _groups(early) == ([], [2, 4, 8])
    _both("R <= 8 only", early, joined, cc.expand(_base(), 2), _ref_base(f), "amplitude")
    early.close(); joined.close()


# ---- several segments -------------------------------------------------------------------------------------------------
def test_two_epochs_in_one_batch():
    n, eb = 40000, [[3, 19001], [19007, 39001]]
    early, joined = _pair(lambda: _plan(n, 2, epoch_bounds=eb))
    assert early.debug_batches() == [(0, 2)] and _groups(early) == ([16, 32, 64, 128], [2, 4, 8])
    _both("two epochs", early, joined, cc.expand(_base(n), 2), _ref_base(n=n, epoch_bounds=eb), "amplitude")
    early.close(); joined.close()


def test_time_blocks_with_reused_means():
    """A recording of 2^18 samples cut into five time blocks (FFTs of 2^16 points), computed block by block through
    execute_block with the channel means of the first request reused, as the streamed configuration does."""
    n, f = 1 << 18, F6[::2]
    early, joined = _pair(lambda: _plan(n, 1, f, max_fft_log2=16))
    segs = early.segments()
    assert len(segs) >= 3 and segs == joined.segments() and _groups(early) == ([16, 32, 64, 128], [2, 4, 8])
    x = np.ascontiguousarray(_base(n)[:1])
    ref = _oracle(("blocks", n), lambda: np.abs(orc.cwt_complex(x[0].astype(np.float64), FS, f, n_threads=8)))
    worst = 0.0
    for i, (a, b, _) in enumerate(segs):
        got = early.execute_block(x, a, b - a, reuse_means=i > 0)
        want = joined.execute_block(x, a, b - a, reuse_means=i > 0)
        assert np.array_equal(got, want), (i, a, b)
        worst = max(worst, float(rel_err(got[0], ref[:, a:b]).max()))
    print("    %d time blocks: worst row %.3g of the row's peak (gate %.0e)" % (len(segs), worst, TOL))
    assert worst <= TOL
    early.close(); joined.close()


# ---- graph replay, repeated executes ----------------------------------------------------------------------------------
def test_graph_replay():
    """A small device-resident plan: the first execute eager, the second captured (branches on the three streams, the
    side streams joined behind k_synthi), the third and fourth replayed; all four the bits of the joined order."""
    from ghost_amd.engine import DeviceBuffer
    c = 2
    early, joined = _pair(lambda: _plan(N, c))
    x = cc.expand(_base(), c)
    want = joined.execute(x)
    xb, ob = DeviceBuffer(4 * c * N), DeviceBuffer(early.info["out_bytes"])
    xb.upload(x)
    outs = []
    for _ in range(4):
        early.execute_device(xb, ob)
        outs.append(ob.download((c, F6.size, N), np.float32))
    assert early.debug_graph_state() == 1
    for i, got in enumerate(outs):
        assert np.array_equal(got, outs[0]), i
    assert np.array_equal(outs[0], want)
    _gate("graph replay", outs[3], _ref_base(), "amplitude")
    xb.free(); ob.free()
    early.close(); joined.close()


def test_twenty_executes_in_a_row():
    """One plan, twenty executes without a graph (a missing join between steps would let a step's level passes run
    into the next step's forward transform), inputs alternating so that a stale buffer shows."""
    from ghost_amd.engine import DeviceBuffer
    c = 2
    with _Options(graphs=0):
        early, joined = _pair(lambda: _plan(N, c))
    xs = [cc.expand(_base(), c), np.ascontiguousarray(cc.expand(_base(), c)[:, ::-1])]
    want = [joined.execute(x) for x in xs]
    xb = [DeviceBuffer(4 * c * N) for _ in xs]
    for b, x in zip(xb, xs):
        b.upload(x)
    ob = DeviceBuffer(early.info["out_bytes"])
    for i in range(20):
        early.execute_device(xb[i & 1], ob)
        assert np.array_equal(ob.download((c, F6.size, N), np.float32), want[i & 1]), i
    assert early.debug_graph_state() == 0
    _gate("twenty executes", want[0], _ref_base(), "amplitude")
    for b in xb + [ob]:
        b.free()
    early.close(); joined.close()


# ---- the other kernel variants ----------------------------------------------------------------------------------------
def test_output_stride():
    """output_stride = 3: the strided kernels behind the same forks and joins."""
    early, joined = _pair(lambda: _plan(N, 2, output_stride=3))
    assert _groups(early) == ([16, 32, 64, 128], [2, 4, 8])
    _both("output_stride = 3", early, joined, cc.expand(_base(), 2), _ref_base()[..., ::3], "amplitude")
    early.close(); joined.close()


def test_morlet_plan():
    """Morlet levels are never interpolated: the joined order, untouched."""
    w0 = 6.0
    early, joined = _pair(lambda: _plan(N, 2, morlet_w0=w0, output="amplitude"))
    assert early.info["n_interp"] == 0
    x = cc.expand(_base(), 2)
    got, want = early.execute(x), joined.execute(x)
    assert np.array_equal(got, want)
    ref = _oracle(("morlet", w0), lambda: np.abs(np.stack([mc.truth(x[ch], FS, F6, w0, threads=8) for ch in range(2)])))
    err = rel_err(got, ref)
    print("    Morlet: worst row %.3g of the row's peak (gate %.0e)" % (err.max(), TOL))
    assert err.max() <= TOL
    early.close(); joined.close()


def test_shifted_bands():
    """Morse(3, 4): every level's band starts below zero frequency, so each stream gathers its slice of the spectrum
    into its own part of the slice buffer; two levels per decimation share an x_R."""
    early, joined = _pair(lambda: _plan(N, 2, gamma=3.0, beta=4.0))
    lv = early.debug_levels()
    assert all(l["band_shift"] > 0 for l in lv) and len(lv) > len({l["decimation"] for l in lv})
    h, low = _groups(early)
    assert h and low and min(h) >= 16 and max(low) <= 8
    _both("Morse(3, 4)", early, joined, cc.expand(_base(), 2), _ref_base(gamma=3.0, beta=4.0), "amplitude")
    early.close(); joined.close()
