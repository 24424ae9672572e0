"""Shared pieces of the channel-count tests (plain module, no fixtures, no GPU): recordings of C channels every one of
which is told apart from every other although the oracle runs on five signals only, what each channel's rows must be,
and the layouts of the cases (tests/test_channel_cases_cpu.py pins the planner's decisions for them,
tests/test_gpu_channel_matrix.py runs them).

Channel c of ``expand(base, C)`` carries s_c 2^k_c base[c % 5], k_c = ((c // 5) % 9) - 4, s_c = -1 where c // 45 is
odd.  A float32 times a power of two is exact, so channel c IS a scaled base; the transform is linear and its mean
removal too, so the rows of channel c are the base's rows times s_c 2^k_c (amplitude: 2^k_c, power: 4^k_c), exactly.
The pattern repeats after 90 channels = 2 x 45: no tile of 8, 16, 32 or 64 channels meets the same data at the same
place twice."""
import numpy as np

from conftest import rel_err
from oracle import ghost_oracle as orc

FS = 1000.0
TOL = 1e-5                      # the project's gate, per row against the row's peak (conftest.rel_err); 2 TOL on power
N_BASE = 5
PERIOD = 90


def gate(output):
    return 2 * TOL if output == "power" else TOL


def exponents(n_channels):
    """(k, s) of every channel: int arrays (C,)."""
    c = np.arange(int(n_channels))
    return (c // N_BASE) % 9 - 4, np.where((c // (9 * N_BASE)) % 2 == 1, -1, 1)


def base_index(n_channels):
    return np.arange(int(n_channels)) % N_BASE


def factors(n_channels, output="complex"):
    """float64 (C,): what the base's rows are multiplied by to give channel c's, by output mode."""
    k, s = exponents(n_channels)
    if output == "complex":
        return s * 2.0 ** k
    return 2.0 ** k if output == "amplitude" else 4.0 ** k


def base_signals(n, seed=1234):
    from ghost_amd.synthetic import lfp
    return lfp(N_BASE, n, FS, seed)


def expand(base, n_channels):
    """float32 (C, n) from float32 (5, n)."""
    base = np.asarray(base)
    assert base.dtype == np.float32 and base.shape[0] == N_BASE
    x = base[base_index(n_channels)] * factors(n_channels).astype(np.float32)[:, None]
    assert x.dtype == np.float32
    return x


def as_output(output, c):
    return c if output == "complex" else np.abs(c) if output == "amplitude" else np.abs(c) ** 2


def oracle_base(base, freqs, output="complex", epoch_bounds=None, **kw):
    """The oracle on the five base signals, as ``output``: float64 / complex128 (5, S, n)."""
    eb = None if epoch_bounds is None else np.asarray(epoch_bounds).reshape(-1, 2)
    return np.stack([as_output(output, orc.cwt_complex(b.astype(np.float64), FS, freqs, eb, **kw)) for b in base])


def expected(ref_base, n_channels, output="complex"):
    """Rows of every channel from the base's rows ``ref_base`` (5, S, n) of the same output mode: (C, S, n)."""
    return ref_base[base_index(n_channels)] * factors(n_channels, output)[:, None, None]


def unscaled(got, output="complex"):
    """``got`` (C, S, n) float32 / complex64 with every channel's factor taken out again: exact (a power of two), same
    dtype.  Channel c then holds what the device made of base[c % 5], had nothing depended on k_c, s_c or c."""
    inv = (1.0 / factors(got.shape[0], output)).astype(np.float32)
    flat = got.view(np.float32) if np.iscomplexobj(got) else got        # (a complex product would add signed zeros)
    return (flat * inv[:, None, None]).view(got.dtype)


def _groups(u):
    """(whole periods of five channels as (G, 5, S, n) -- a view --, the C % 5 channels left over)."""
    whole = u.shape[0] // N_BASE * N_BASE
    return u[:whole].reshape((-1, N_BASE) + u.shape[1:]), u[whole:]


def homogeneous(got, output="complex", source=None):
    """True when every channel, its factor taken out, holds the bits of the first channel of its base -- hence of the
    channel of that base with k = 0, s = +1 too.  Every channel, row and column; no copy of the result but one.
    ``source`` (C,): which signal channel c is a scaled copy of, where that is not c % 5 (bad_electrodes)."""
    if source is not None:
        u = unscaled(got, output)
        _, first, inverse = np.unique(source, return_index=True, return_inverse=True)
        return bool(np.array_equal(u, u[first[inverse]]))
    groups, rest = _groups(unscaled(got, output))
    if groups.shape[0] == 0:                                  # fewer than six channels: no base comes twice
        return True
    return bool(np.array_equal(groups, np.broadcast_to(groups[:1], groups.shape)) and
                np.array_equal(rest, groups[0, :rest.shape[0]]))


def oracle_error(got, ref_base, output="complex", chunk=128, source=None):
    """rel_err(got[c], expected[c]) of every row of every channel, (C, S), without building ``expected``: the factor is
    a power of two, so rel_err(got[c], f_c ref) == rel_err(got[c] / f_c, ref) to the bit.  ``chunk`` groups of five
    channels at a time bound the float64 temporaries.  ``source`` (C,): rows of ``ref_base`` by channel, as above."""
    if source is not None:
        u = unscaled(got, output)
        return np.concatenate([rel_err(u[c:c + 5], ref_base[source[c:c + 5]]) for c in range(0, u.shape[0], 5)])
    groups, rest = _groups(unscaled(got, output))
    err = [rel_err(groups[g:g + chunk], ref_base) for g in range(0, groups.shape[0], chunk)]
    err = np.concatenate(err).reshape(-1, ref_base.shape[1]) if err else np.zeros((0, ref_base.shape[1]))
    if rest.shape[0]:
        err = np.concatenate([err, rel_err(rest, ref_base[:rest.shape[0]])])
    return err


def picks(n_channels):
    """The channels compared with a one-channel plan: first, middle, last."""
    return sorted({0, n_channels // 2, n_channels - 1})


# ---- the cases' layouts --------------------------------------------------------------------------------------------
A_N = 20000
A_F = np.geomspace(300.0, 2.0, 16)
A_INTERP = {16: (2, 8), 32: (4, 8), 64: (4, 16), 128: (4, 32)}          # decimation: (q, I) of the interpolated levels

B_N = 8000
B_EPOCHS = [[400 * i, 400 * i + 300 + 7 * (i % 5)] for i in range(20)]
B_F = [320.0, 140.0, 61.0]
B_BATCH_BYTES = 64 << 30


def b_block(first_batch):
    """(start, length) of a block request that starts inside the last epoch of a first batch of ``first_batch`` epochs
    and ends inside the second epoch of the next batch: 5850 .. 6500 for 15."""
    return 400 * first_batch - 150, 650


C_F = [100.0, 60.0, 391.0]
C_LIMIT = dict(n_channels=65535, n=600, epochs=[[0, 250], [300, 600]])
C_ROWS = dict(n_channels=21846, n=1200, epochs=[[0, 250], [300, 600], [650, 900], [950, 1200]])

D_N = 12000
D_F = [300.0, 140.0, 61.0, 33.0, 17.0, 9.0]
D_EPOCHS = [[50, 7000], [7011, 12000]]
D_MORLET_N = 20000
D_MORLET_W0 = 6.0

E_N = 200000
E_F = np.geomspace(200.0, 2.0, 12)
E_LINE = 300.0                                                          # the line's amplitude over the channel's spread

F_N = 5003
F_F = np.geomspace(200.0, 4.0, 6)


def morlet_freqs():
    """Every third frequency of the grid transform() builds for Morlet(w0 = 6) on 20 000 samples (morlet_cases:
    default_grid), which runs from the time-domain scales down to decimation 16 and beyond."""
    import morlet_cases as mc
    return mc.default_grid(D_MORLET_W0, D_MORLET_N, FS)[::3]


def inside(n, epochs):
    """bool (n,): the samples of some epoch."""
    m = np.zeros(n, bool)
    for a, b in epochs:
        m[a:b] = True
    return m


def bad_electrodes(base, n_channels, dirty, amp=E_LINE):
    """(x float32 (C, n), sources float32 (10, n), source index (C,)): ``expand`` with a windowed 60 Hz line of ``amp``
    times the base's spread added to the bases of the channels ``dirty`` BEFORE the scaling, so that a dirty channel is
    a scaled copy of one of five dirty bases: sources 0..4 clean, 5..9 with the line."""
    n = base.shape[1]
    line = np.sin(np.pi * np.arange(n) / n) ** 2 * np.sin(2 * np.pi * 60.0 * np.arange(n) / FS)
    b64 = base.astype(np.float64)
    sources = np.concatenate([base, (b64 + amp * b64.std(axis=1, keepdims=True) * line).astype(np.float32)])
    src = base_index(n_channels) + N_BASE * np.isin(np.arange(n_channels), dirty)
    x = sources[src] * factors(n_channels).astype(np.float32)[:, None]
    return x, sources, src
