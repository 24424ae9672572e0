"""Shared pieces of the interpolating-synthesis tests (plain module, no fixtures, no GPU): the cases that between them
reach every data-dependent branch of k_synthi (csrc/synthi.hip), what a plan reaches read off the planner's hooks, a
restatement of how work_items.cpp cuts a level into workgroup items, and the float64 model / oracle rows of a case, computed
once (tests/test_synthi_cases_cpu.py pins the planner's decisions, tests/test_gpu_synthi_matrix.py runs the cases).

Case   plan                                                        what it is there for
B      1 kHz, 2^17 samples, geomspace(20, 0.2, 24)                 q = 2 at R = 16 (8 taps, one scale: n_scales < ns),
                                                                   q = 4 / 6 taps at R = 32 .. 1024, I = 8 .. 256
B2     the same grid on two epochs of one FFT length, bounds and   `lead`, a batch of two segments, windows over a gap
       gap multiples of neither 4 nor 64
C      30 kHz, 2^21 samples, geomspace(200, 1, 20)                 R = 64 .. 8192, I = 512 and 1024 (the coefficient
                                                                   class depends on wt mod 4), q = 8, passes shared
                                                                   among workgroups (parts > 1)
D      30 kHz, 2^22 samples, geomspace(4, 0.5, 8)                  q = 16 at R = 16384, two time-block segments
E      Morse(3, 8), 1 kHz, 1e5 samples, sixteen drawn frequencies  the eight-tap fallback of q = 4 (R = 64, 512), a level
                                                                   the design refuses (R = 16 stays on k_synth7)
F34    Morse(3, 4), 1 kHz, 60 000 samples, geomspace(100, 1.5, 20) shifted bands, halos 44 .. 69, two levels per R
F28    Morse(2, 8), the same grid                                  shifted bands (shift 113 .. 120)

The time blocks of case D (segments with a faded halo of input on either side, level grids shared by the batch) are
not in the float64 model: its rows go against the oracle alone."""
import numpy as np

from decimated_model import amplitude_interpolated, level_of_scale
from oracle import ghost_oracle as orc

GATE = 1e-5                     # the project's gate against the oracle (conftest.rel_err)
MODEL_CPU = 1e-6                # model against oracle, every row (planner: 2e-7 + band_tol; worst measured 3.5e-7)
K_COLS = 16                     # interp.h: kInterpCols, the columns of a pass
HOST_GAIN_FROM = 1 << 20        # taps from which the model takes G from the library's host evaluation


def _e_freqs():
    rng = np.random.default_rng(18)
    rng.uniform(size=16)                  # (the list that was found is the generator's second sixteen draws)
    return np.sort(np.exp(rng.uniform(np.log(0.5), np.log(40.0), 16)))[::-1].copy()


CASES = {
    "B": dict(fs=1000.0, n=1 << 17, f=np.geomspace(20.0, 0.2, 24), gamma=3.0, beta=20.0, epochs=None, channel=3),
    "B2": dict(fs=1000.0, n=116005, f=np.geomspace(20.0, 0.2, 24), gamma=3.0, beta=20.0,
               epochs=[[3, 58001], [58007, 116001]], channel=4),
    "C": dict(fs=30000.0, n=1 << 21, f=np.geomspace(200.0, 1.0, 20), gamma=3.0, beta=20.0, epochs=None, channel=5),
    "D": dict(fs=30000.0, n=1 << 22, f=np.geomspace(4.0, 0.5, 8), gamma=3.0, beta=20.0, epochs=None, channel=6),
    "E": dict(fs=1000.0, n=100000, f=_e_freqs(), gamma=3.0, beta=8.0, epochs=None, channel=7),
    "F34": dict(fs=1000.0, n=60000, f=np.geomspace(100.0, 1.5, 20), gamma=3.0, beta=4.0, epochs=None, channel=8),
    "F28": dict(fs=1000.0, n=60000, f=np.geomspace(100.0, 1.5, 20), gamma=2.0, beta=8.0, epochs=None, channel=9),
}
CUT_CASES = ("B", "C", "F28")                            # the cases the GPU file runs under every forced work cut
MODELLED = ("B", "B2", "C", "E", "F34", "F28")          # every case but the time-block one

# decimation: (q, I, taps) of every level of the case, None where the design refuses it (k_synth7), in plan order
DESIGNS = {
    "B": [(16, (2, 8, 8)), (32, (4, 8, 6)), (64, (4, 16, 6)), (128, (4, 32, 6)), (256, (4, 64, 6)), (512, (4, 128, 6)),
          (1024, (4, 256, 6))],
    "B2": [(16, (2, 8, 8)), (32, (4, 8, 6)), (64, (4, 16, 6)), (128, (4, 32, 6)), (256, (4, 64, 6)), (512, (4, 128, 6))],
    "C": [(64, (4, 16, 6)), (128, (4, 32, 6)), (256, (4, 64, 6)), (512, (4, 128, 6)), (1024, (4, 256, 6)),
          (2048, (4, 512, 6)), (4096, (4, 1024, 6)), (8192, (8, 1024, 6))],
    "D": [(4096, (4, 1024, 6)), (8192, (8, 1024, 6)), (16384, (16, 1024, 6))],
    "E": [(16, None), (32, (4, 8, 6)), (64, (4, 16, 8)), (512, (4, 128, 8))],
    "F34": [(2, None), (2, None), (4, None), (4, None), (8, None), (8, None), (16, (2, 8, 8)), (16, (2, 8, 8)),
            (32, (4, 8, 6)), (32, (4, 8, 6))],
    "F28": [(2, None), (4, None), (8, None), (16, (2, 8, 8)), (32, (4, 8, 6)), (64, (4, 16, 6))],
}


def signal(name):
    """float32 (n,): the case's recording."""
    from ghost_amd.synthetic import lfp_channel
    c = CASES[name]
    return np.ascontiguousarray(lfp_channel(c["n"], c["fs"], channel=c["channel"]), dtype=np.float32).reshape(-1)


def make_plan(name, output="amplitude", n_channels=1):
    from ghost_amd.engine import CwtPlan
    c = CASES[name]
    return CwtPlan(c["n"], n_channels, c["fs"], c["f"], gamma=c["gamma"], beta=c["beta"], epoch_bounds=c["epochs"],
                   output=output)


def epochs_of(name):
    c = CASES[name]
    return np.array([[0, c["n"]]] if c["epochs"] is None else c["epochs"])


def taps_of(design):
    """6 where the outer two of the table's eight columns are zero (planner.cpp: the middle six), else 8."""
    coef = design["coef"]
    return 6 if not coef[:, :, 0].any() and not coef[:, :, 7].any() else 8


def designs(plan):
    """[(decimation, (q, I, taps) or None)] per level, plan order."""
    return [(lv["decimation"], None if d is None else (d["q"], d["factor"], taps_of(d)))
            for lv, d in zip(plan.debug_levels(), plan.debug_interp()["levels"])]


def clamp_lgnb(decimation, q, lgnb=None):
    """Blocks per workgroup (log2) of a level: work_items.cpp's default, the forced value of option interp_lgnb, and the
    clamp (q << lgnb) <= 16 (synthi_items, "Blocks per workgroup")."""
    v = (1 if decimation <= 32 and q <= 2 else 0) if lgnb is None else min(int(lgnb), 2)
    while v > 0 and (q << v) > K_COLS:
        v -= 1
    return v


def walk(parities, q, lgnb):
    """Parity of the scale the kernel's pass B visits, z slot by z slot, pass by pass (synthi.hip: zi -> slot
    zi & (ns - 1) of block zi >> lgns; slots past the level's last scale are skipped).  The level's list holds the odd
    kernel lengths first, so the list itself switches at most once; a pass that straddles the switch is walked once per
    block of the group."""
    nb = 1 << lgnb
    ns = K_COLS // (q * nb)
    seq = []
    for b0 in range(0, len(parities), ns):
        for zi in range(K_COLS // q):
            sl = zi & (ns - 1)
            if b0 + sl < len(parities):
                seq.append(parities[b0 + sl])
    return seq


def switches(seq):
    return int(sum(a != b for a, b in zip(seq[:-1], seq[1:])))


def items(plan, lgnb=None, batch=0):
    """RESTATEMENT of how synthi_items (csrc/work_items.cpp, "A workgroup walks all the scales of its blocks unless
    that is too much for one"; cut_largest_first halves `target`) cuts the interpolated levels of one launch batch
    into workgroup items.  A change to that cut must change this too: tests/test_synthi_cases_cpu.py holds the two
    together through ``debug_work_items``.  Used only to assert that a case has items
    of several parts, items that start after the level's first pass and levels walked in one pass, and to place test
    windows inside / across the parts.

    Returns (items, target): items as dicts level, decimation, blk0, pass0, n_pass, lo, hi (wave-tasks of 256 samples),
    parts, run, wps; in the order of the loop, not sorted by size."""
    first, count = plan.debug_batches()[batch]
    levels = plan.debug_levels(epoch=first)
    di = plan.debug_interp()["levels"]
    lof = level_of_scale(plan)
    n_ch_slots = plan.n_channels * max(1, count)
    pending = sorted((l for l, d in enumerate(di) if d is not None), key=lambda l: -levels[l]["decimation"])
    target = 2 << 20
    attempt = 0
    while True:
        out = []
        for l in pending:
            lv, q = levels[l], di[l]["q"]
            nb = 1 << clamp_lgnb(lv["decimation"], q, lgnb)
            ns = K_COLS // (q * nb)
            n_scales = int((lof == l).sum())
            n_pass = (n_scales + ns - 1) // ns
            pass_bytes = ns * nb * lv["hop"] * lv["decimation"] * 4
            run = max(1, min(n_pass, target // max(1, pass_bytes)))
            wps = (lv["hop"] * (lv["decimation"] >> 2) + 63) >> 6
            quads = (wps + 3) // 4
            parts = 1 if run > 1 else min(quads, (pass_bytes + target - 1) // target)
            for b0 in range(0, lv["nblk"], nb):
                for p0 in range(0, n_pass, run):
                    for part in range(parts):
                        out.append(dict(level=l, decimation=lv["decimation"], blk0=b0, pass0=p0,
                                        n_pass=min(run, n_pass - p0), lo=4 * (quads * part // parts),
                                        hi=min(wps, 4 * (quads * (part + 1) // parts)), parts=parts, run=run, wps=wps))
        if len(out) * n_ch_slots >= 3072 or target <= (1 << 19) or attempt > 6:
            return out, target
        target >>= 1
        attempt += 1


def branches(plan):
    """What a plan reaches in k_synthi, per interpolated level (keyed by the level's index in ``debug_levels``): the
    design, lgi4 (I / 4 = 1 << lgi4), the rows in the kernel's list order with their parities, per interp_lgnb in
    (None, 0, 1, 2) the cut of the walk (ns scales per pass, the ragged remainder, blocks per group, switches of the
    coefficient table in walk order), the band shift and halo, and the level's items under the default cut."""
    si, levels = plan.scale_info(), plan.debug_levels()
    di = plan.debug_interp()["levels"]
    lof = level_of_scale(plan)
    its, _ = items(plan)
    res = {}
    for l, (lv, d) in enumerate(zip(levels, di)):
        if d is None:
            continue
        rows = np.flatnonzero(lof == l)
        even = (si["length"][rows] % 2 == 0)
        rows = np.concatenate([rows[~even], rows[even]])              # work_items.cpp: odd kernel lengths first
        par = [int(si["length"][r] % 2 == 0) for r in rows]
        lgi4 = int(np.log2(d["factor"] // 4))
        cut = {}
        for opt in (None, 0, 1, 2):
            lgnb = clamp_lgnb(lv["decimation"], d["q"], opt)
            nb = 1 << lgnb
            ns = K_COLS // (d["q"] * nb)
            cut[opt] = dict(lgnb=lgnb, nb=nb, ns=ns, n_pass=-(-len(rows) // ns), ragged=len(rows) % ns,
                            ragged_blocks=lv["nblk"] % nb, switches=switches(walk(par, d["q"], lgnb)))
        res[l] = dict(decimation=lv["decimation"], q=d["q"], factor=d["factor"], taps=taps_of(d), lgi4=lgi4,
                      halo=lv["halo"], hop=lv["hop"], nblk=lv["nblk"], shift=lv["band_shift"], rows=rows.tolist(),
                      parities=par, cut=cut, items=[it for it in its if it["level"] == l])
    return res


def interpolated_rows(plan):
    """Rows k_synthi writes, and rows of decimated levels the design refused (k_synth7 in an amplitude plan)."""
    lof = level_of_scale(plan)
    di = plan.debug_interp()["levels"]
    on = np.array([l >= 0 and di[l] is not None for l in lof])
    return np.flatnonzero(on), np.flatnonzero((lof >= 0) & ~on)


_CACHE = {}


def model(name):
    """float64 (S, n): the model's amplitude rows of a case (decimated_model.amplitude_interpolated), made once."""
    key = ("model", name)
    if key not in _CACHE:
        c = CASES[name]
        plan = make_plan(name)
        out = amplitude_interpolated(signal(name), c["fs"], c["f"], epochs_of(name), c["gamma"], c["beta"], plan=plan,
                                     host_gain_from=HOST_GAIN_FROM)
        out.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def oracle(name, n_threads=8):
    """float64 (S, n): |W| of the literal reference path, made once."""
    key = ("oracle", name)
    if key not in _CACHE:
        c = CASES[name]
        out = np.abs(orc.cwt_complex(signal(name).astype(np.float64), c["fs"], c["f"], epochs_of(name), c["gamma"],
                                     c["beta"], n_threads=n_threads))
        out.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]
