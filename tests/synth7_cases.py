"""Shared pieces of the k_synth7 stage tests (plain module, no fixtures, no GPU): the cases that between them reach every
data-dependent branch of k_synth7 (csrc/synth.hip; its complex-gain build in synth_morlet.hip), what a plan reaches
read off the planner's hooks, and the float64 model of the stage on its own -- steps 3 and 4 of DESIGN.md section 3
from a level's x_R (decimated_model.synth_stage), with the exact gains (tests/test_synth7_cases_cpu.py pins the
planner's decisions and checks the model, tests/test_gpu_synth7_matrix.py runs the cases on the device's own x_R;
profiles/synth7_matrix.md has the measurements).

Case    plan (1 kHz, Morse(3, 20) unless said)                     what it is there for
A1      30 000 samples, 32 drawn frequencies, R = 2, 4, 8          levels of 9, 16, 7 scales; the ramp at 8 of 9 (a chunk's
                                                                   first scale, the level's last), 8 of 16, 3 of 7
A2      the same, 26 frequencies                                   levels of 1, 17, 8 scales; ramp never (1 of 1, 8 of 8),
                                                                   at 0 of 17
C1, C2  A1, A2 and levels at R = 16, 32; complex only              levels of 17, 1 and 16, 9 scales more (ramp at 8 of 17,
                                                                   0 of 1, 11 of 16, 8 of 9); R = 32 is two phase tiles of
                                                                   the 16-column build
A256    12 000 samples, geomspace(68, 38, 256)                     one level of 256 scales (32 chunks), ramp at 127
A255    the same without the last scale                            a ragged last chunk of 7
M6, M4  Morlet w0 = 6 (unshifted) and 4 (shifted, halo 35 / 36),   chunks of 4: levels of 9, 8, 5, 4, 3, 1 scales, complex
        30 000 samples                                             rows, no ramp
W       2^18 samples, geomspace(8, 0.05, 14); complex              R = 64 .. 4096: 2 .. 128 phase tiles of 32 columns (4 ..
                                                                   256 of 16), levels of one block
H16 ..  1 500 samples, [100, f]: the cap on R (16) makes the halo  halo 16, 17, 31, 32, 33, 47, 48 at R = 16: every lane class
H48     of the second scale a function of f                        of keep1 / keep14 / keep2 / keep13
HW      Morse(3, 4), 30 000 samples, geomspace(120, 20, 10)        shifted bands, halo 46 and 66 (the WIDE instantiation)
S       C1 (complex) / A1 (amplitude) on two epochs of one FFT     `lead` 3 and 55, a batch of two segments, three
        length, odd bounds, a gap that is no multiple of 4         channels: slot = segment x channels + channel
                                                                   (own recordings); groups of blocks of the shorter
                                                                   segment leave early at R = 2 .. 16, both column builds

Amplitude plans of the H cases are made under option interp = 0: at R = 16 the planner would otherwise send the level to
k_synthi (tests/synthi_cases.py).  The long-mode and time-block layouts stay with the oracle-only tests."""
import numpy as np

import morlet_cases as mc
import morlet_model
from decimated_model import exact_gain, level_input, synth_stage
from oracle import ghost_oracle as orc

GATE = 1e-5                     # the project's gate against the oracle (conftest.rel_err); twice for power
MODEL_CPU = 1e-6                # model against oracle, every row (synthi_cases.MODEL_CPU)
STAGE_CAP = 1e-6                # device rows against the stage model: the bound never exceeds this
HOST_GAIN_FROM = 1 << 14        # taps from which the model takes G from the library's host evaluation
BAND_TOL = 2e-7                 # planner.cpp: hp->band_tol, what k_scale_windows prunes the first layer by
B = 256

DENSE = np.geomspace(200.0, 1.5, 400)           # the grid the Morse and Morlet lists were drawn from (indices below)
# found by planning DENSE and taking, per decimation, the wanted numbers of odd and even kernel lengths spread evenly
_A1 = [1, 5, 8, 11, 12, 16, 19, 21, 25, 26, 28, 32, 37, 39, 44, 47, 52, 56, 60, 63, 66, 70, 74, 79, 82, 83, 84, 104,
       108, 122, 136, 138]
_A2 = [14, 26, 29, 31, 34, 35, 38, 41, 44, 48, 52, 53, 59, 61, 62, 76, 77, 79, 83, 91, 96, 105, 111, 118, 126, 138]
_C1 = _A1 + [139, 140, 146, 148, 152, 156, 160, 165, 167, 169, 176, 178, 182, 187, 188, 193, 195, 234]
_C2 = _A2 + [139, 140, 145, 151, 152, 156, 159, 162, 169, 170, 178, 182, 185, 190, 193, 195, 197, 202, 207, 218, 225,
             230, 234, 242, 252]


def _spread(lo, hi, n):
    """n indices of lo .. hi (inclusive) spread evenly; the middle one for n = 1."""
    return [(lo + hi) // 2] if n == 1 else np.round(np.linspace(lo, hi, n)).astype(int).tolist()


# Morlet: a level is a run of DENSE (w0 = 6: R = 2 is 0 .. 34, R = 4 35 .. 90, ...; w0 = 4: R = 2 is 23 .. 78, ...)
_M6 = sum((_spread(a, b, n) for a, b, n in ((0, 34, 1), (35, 90, 9), (91, 147, 8), (148, 203, 5), (204, 260, 4),
                                            (261, 316, 3))), [])
_M4 = sum((_spread(a, b, n) for a, b, n in ((23, 78, 9), (79, 135, 8), (136, 191, 5), (192, 248, 4), (249, 305, 3),
                                            (306, 363, 1))), [])
H_FREQS = {16: 30.0, 17: 25.0, 31: 12.8, 32: 12.37, 33: 11.92, 47: 8.15, 48: 7.95}     # halo at R = 16: second frequency
S_EPOCHS = [[3, 14001], [14007, 22997]]


def _case(n, f, outputs, gamma=3.0, beta=20.0, w0=None, epochs=None, channels=(1,), interp0=False):
    return dict(fs=1000.0, n=n, f=np.asarray(f, dtype=np.float64), outputs=outputs, gamma=gamma, beta=beta, w0=w0,
                epochs=epochs, channels=channels, interp0=interp0)


_ALL = ("complex", "amplitude", "power")
CASES = {
    "A1": _case(30000, DENSE[_A1], _ALL),
    "A2": _case(30000, DENSE[_A2], _ALL),
    "C1": _case(30000, DENSE[_C1], ("complex",)),
    "C2": _case(30000, DENSE[_C2], ("complex",)),
    "A256": _case(12000, np.geomspace(68.0, 38.0, 256), ("complex", "amplitude")),
    "A255": _case(12000, np.geomspace(68.0, 38.0, 256)[:255], ("complex", "amplitude")),
    "M6": _case(30000, DENSE[_M6], ("complex", "amplitude"), w0=6.0),
    "M4": _case(30000, DENSE[_M4], ("complex", "amplitude"), w0=4.0),
    "W": _case(1 << 18, np.geomspace(8.0, 0.05, 14), ("complex",)),
    "HW": _case(30000, np.geomspace(120.0, 20.0, 10), ("complex", "amplitude"), beta=4.0),
    "S": _case(30000, DENSE[_C1], ("complex",), epochs=S_EPOCHS, channels=(3,)),
    "Sa": _case(30000, DENSE[_A1], ("amplitude",), epochs=S_EPOCHS, channels=(3,)),
}
FAMILY = {"A1": "A", "A2": "A", "C1": "A", "C2": "A", "A256": "A256", "A255": "A256", "M6": "M", "M4": "M", "W": "W",
          "HW": "H", "S": "S", "Sa": "S"}


for _halo, _f in H_FREQS.items():
    CASES["H%d" % _halo] = _case(1500, [100.0, _f], ("complex", "amplitude"), interp0=True)
    FAMILY["H%d" % _halo] = "H"


# level table of every case: (decimation, halo, hop, blocks of epoch 0, band shift, scales, n_plain, kernel), the levels
# that hold scales in plan order -- what tests/test_synth7_cases_cpu.py pins
_K, _KW = "k_synth7", "k_synth7w"
_A1_LV = [(2, 22, 212, 71, 0, 9, 8, _K), (4, 22, 212, 36, 0, 16, 8, _K), (8, 22, 212, 18, 0, 7, 3, _K)]
_A2_LV = [(2, 20, 216, 70, 0, 1, 1, _K), (4, 21, 214, 36, 0, 17, 0, _K), (8, 22, 212, 18, 0, 8, 8, _K)]
_S_LV = [(2, 22, 212, 34, 0, 9, 8, _K), (4, 22, 212, 17, 0, 16, 8, _K), (8, 22, 212, 9, 0, 7, 3, _K)]
EXPECT = {
    "A1": _A1_LV,
    "A2": _A2_LV,
    "C1": _A1_LV + [(16, 22, 212, 9, 0, 17, 8, _K), (32, 18, 220, 5, 0, 1, 0, _K)],
    "C2": _A2_LV + [(16, 22, 212, 9, 0, 16, 11, _K), (32, 22, 212, 5, 0, 9, 8, _K)],
    "A256": [(8, 21, 214, 8, 0, 256, 127, _K)],
    "A255": [(8, 21, 214, 8, 0, 255, 127, _K)],
    "M6": [(2, 18, 220, 69, 0, 1, 1, _K), (4, 20, 216, 35, 0, 9, 9, _K), (8, 20, 216, 18, 0, 8, 8, _K),
           (16, 20, 216, 9, 0, 5, 5, _K), (32, 20, 216, 5, 0, 4, 4, _K), (64, 20, 216, 3, 0, 3, 3, _K)],
    "M4": [(2, 36, 184, 82, 73, 9, 9, _K), (4, 35, 186, 41, 73, 8, 8, _K), (8, 35, 186, 21, 73, 5, 5, _K),
           (16, 35, 186, 11, 73, 4, 4, _K), (32, 35, 186, 6, 74, 3, 3, _K), (64, 26, 204, 3, 52, 1, 1, _K)],
    "W": [(64, 19, 218, 19, 0, 2, 1, _K), (128, 21, 214, 10, 0, 2, 2, _K), (256, 32, 192, 6, 0, 3, 3, _K),
          (1024, 18, 220, 2, 0, 2, 2, _K), (2048, 20, 216, 1, 0, 2, 2, _K), (4096, 31, 194, 1, 0, 3, 1, _K)],
    "HW": [(2, 46, 164, 92, 75, 1, 0, _K), (2, 66, 124, 121, 75, 2, 0, _KW), (4, 41, 174, 44, 83, 1, 0, _K)],
    "S": _S_LV + [(16, 22, 212, 5, 0, 17, 8, _K), (32, 18, 220, 2, 0, 1, 0, _K)],
    "Sa": _S_LV,
}
_H_HOP = {16: 224, 17: 222, 31: 194, 32: 192, 33: 190, 47: 162, 48: 160}
_H_PLAIN = {16: 1, 17: 0, 31: 0, 32: 0, 33: 1, 47: 0, 48: 1}
for _halo in H_FREQS:
    EXPECT["H%d" % _halo] = [(4, 17, 222, 2, 0, 1, 0, _K), (16, _halo, _H_HOP[_halo], 1, 0, 1, _H_PLAIN[_halo], _K)]


def signal(name, channel=0):
    """float32 (n,): the case's recording for one channel (each channel its own)."""
    from ghost_amd.synthetic import lfp_channel
    c = CASES[name]
    seed = 11 + sorted(CASES).index(name)
    return np.ascontiguousarray(lfp_channel(c["n"], c["fs"], channel=seed + 7 * channel), dtype=np.float32).reshape(-1)


def make_plan(name, output="complex", n_channels=None):
    """A CwtPlan of the case.  Cases with ``interp0`` need option interp = 0 set around this call for amplitude / power
    (``plan_options``)."""
    from ghost_amd.engine import CwtPlan
    c = CASES[name]
    kw = dict(morlet_w0=c["w0"]) if c["w0"] is not None else dict(gamma=c["gamma"], beta=c["beta"])
    return CwtPlan(c["n"], c["channels"][0] if n_channels is None else n_channels, c["fs"], c["f"],
                   epoch_bounds=c["epochs"], output=output, **kw)


def plan_options(name, output):
    """Options a plan of the case must be made under: {"interp": 0} for the amplitude / power plans of the H cases."""
    return {"interp": 0} if CASES[name]["interp0"] and output != "complex" else {}


def epochs_of(name):
    c = CASES[name]
    return np.array([[0, c["n"]]] if c["epochs"] is None else c["epochs"])


def levels(plan):
    """The plan's levels that hold scales (morlet_cases.levels: found by (decimation, halo, hop)), each with its index
    "level" into ``debug_levels``, "rows" in the kernel's list order, "n_plain", "j_hi" (zeros before the plan's tables
    are on the device) and "kernel"."""
    all_lv = plan.debug_levels()
    lists = plan.debug_scale_lists()
    out = []
    for lv in mc.levels(plan):
        l = [i for i, a in enumerate(all_lv) if (a["decimation"], a["halo"], a["hop"]) == (lv["decimation"], lv["halo"], lv["hop"])]
        assert len(l) == 1
        lv.update(level=l[0], rows=lists[l[0]]["rows"], n_plain=lists[l[0]]["n_plain"], j_hi=lists[l[0]]["j_hi"],
                  kernel=mc.kernel(lv))
        assert sorted(lv["rows"].tolist()) == lv["scales"].tolist()
        out.append(lv)
    return out


def table(plan):
    return [(lv["decimation"], lv["halo"], lv["hop"], lv["nblk"], lv["band_shift"], int(lv["scales"].size), lv["n_plain"],
             lv["kernel"]) for lv in levels(plan)]


def ramp_position(n_scales, n_plain, chunk=8):
    """Where ``b == n_plain`` falls in the walk: "start", "never", "chunk" (a chunk's first scale) or "inside"."""
    if n_plain == n_scales:
        return "never"
    return "start" if n_plain == 0 else "chunk" if n_plain % chunk == 0 else "inside"


def phase_tiles(decimation, cols):
    return max(1, decimation // cols)


def block_groups(lv, cols):
    """Workgroups along the blocks of a level (work_items.cpp: bpb = max(1, cols / R))."""
    bpb = max(1, cols // lv["decimation"])
    return -(-lv["nblk"] // bpb), lv["nblk"] % bpb


def early_groups(plan, cols, narrow_r=2):
    """RESTATEMENT of the test a k_synth7 workgroup makes first (synth.hip: "leave at once if this group of blocks keeps
    no sample inside this segment's window") and of how work_items.cpp cuts a level into groups of blocks: per level that
    holds scales {decimation: [groups of segment 0, 1, ... that leave, of how many]}.  The level grids are those of
    the batch (the union of its segments' own), a segment's window is [lead, lead + its samples), a group of
    max(1, columns / R) blocks keeps the samples [blk0 hop R, (blk0 + blocks) hop R); levels up to ``narrow_r`` take
    the 16-column build in a 32-column plan (option synth7_narrow_r).  Whole epochs of one batch only."""
    assert plan.debug_batches() == [(0, len(plan.segments()))]
    out = {}
    for lv in levels(plan):
        R, span = lv["decimation"], lv["hop"] * lv["decimation"]
        c = 16 if cols == 32 and R <= narrow_r and lv["halo"] <= 48 else cols
        bpb = max(1, c // R)
        firsts = np.arange(0, lv["nblk"], bpb) * span
        gone = []
        for start, stop, _ in plan.segments():
            w_lo = int(start - (start & ~63))
            w_hi = w_lo + int(stop - start)
            gone.append(int(((firsts + bpb * span <= w_lo) | (firsts >= w_hi)).sum()))
        out[R] = (gone, int(firsts.size))
    return out


def lane_classes(halo):
    """How many of the sixteen m2 lanes keep rows 1, 14 (halo <= 32) or 2, 13 (32 < halo <= 48) of their 16 outputs
    (synth.hip: keep1 / keep14 / keep2 / keep13)."""
    m2 = np.arange(16)
    deep = halo > 32
    return dict(keep1=int((~np.bool_(deep) & (m2 >= halo - 16)).sum()), keep14=int((~np.bool_(deep) & (m2 < 32 - halo)).sum()),
                keep2=int((np.bool_(not deep) | (m2 >= halo - 32)).sum()), keep13=int((np.bool_(not deep) | (m2 < 48 - halo)).sum()))


def response(name, plan, i, lv):
    """H_s[k], k < 256, of scale i on its level's grid, frequency (k - shift) / (256 R): the exact response of the
    reference's kernel (decimated_model.exact_gain; the library's host evaluation of the same closed form from
    HOST_GAIN_FROM taps up), or the Morlet closed form of tests/morlet_model.py."""
    c = CASES[name]
    k = np.arange(B) - lv["band_shift"]
    theta = 2 * np.pi * k / (B * lv["decimation"])
    if c["w0"] is not None:
        return morlet_model.response(theta, c["w0"], c["f"][i], c["fs"])
    L = int(plan.scale_info()["length"][i])
    if L >= HOST_GAIN_FROM:
        G = plan.debug_exact_gain(i, k, B * lv["decimation"])
    else:
        G = exact_gain(theta, orc.hz_to_rad(c["f"][i], c["fs"]), L, c["gamma"], c["beta"])
    return G * np.exp(-1j * theta * ((L - 1) / 2 - (L - 1) // 2))


def predicted_j_hi(name, plan, lv):
    """j_hi of every entry of a level's list from the float64 response (kernels.hip: k_scale_windows works on the
    float32 bank; an entry whose last bin above the tolerance sits on a boundary of sixteen may differ by one)."""
    out = []
    for i in lv["rows"]:
        g = np.abs(response(name, plan, int(i), lv))
        out.append(min(16, max(9, (int(np.flatnonzero(g > BAND_TOL * g.max())[-1]) + 16) >> 4)))
    return np.array(out)


def stage_model(name, plan, xr_of, rows=None):
    """complex128 (S, n): every k_synth7 row of one channel from the levels' x_R -- ``xr_of(epoch, level)``: complex
    (M,), ``level_input`` of the float64 spectrum or what the device holds over the FFT length.  Rows that are not on
    a k_synth7 level (or not in ``rows``) stay zero."""
    c = CASES[name]
    out = np.zeros((len(c["f"]), c["n"]), dtype=np.complex128)
    lvs = levels(plan)
    H = {int(i): response(name, plan, int(i), lv) for lv in lvs if lv["kernel"].startswith("k_synth7")
         for i in lv["rows"] if rows is None or int(i) in rows}
    for e, (start, stop) in enumerate(epochs_of(name)):
        lead = int(start - (start & ~63))
        for lv in lvs:
            if not lv["kernel"].startswith("k_synth7"):
                continue
            xr = None
            for i in lv["rows"]:
                if int(i) not in H:
                    continue
                xr = xr_of(e, lv["level"]) if xr is None else xr
                out[i, start:stop] = synth_stage(xr, H[int(i)], lv["band_shift"], lv["decimation"], lv["halo"], lv["hop"],
                                                 lead, int(stop - start))
    return out


def host_levels(name, plan, channel=0):
    """``xr_of`` for ``stage_model`` from the float64 spectrum of the recording (decimated_model.level_input)."""
    from scipy.fft import fft
    x = signal(name, channel).astype(np.float64)
    x = x - x.mean()
    fft_len = {(a, b): p for (a, b, p) in plan.segments()}
    all_lv = plan.debug_levels()
    cache = {}

    def xr_of(e, level):
        start, stop = epochs_of(name)[e]
        if e not in cache:
            lead = int(start - (start & ~63))
            cache[e] = fft(np.concatenate([np.zeros(lead), x[start:stop]]), n=fft_len[(start, stop)])
        return level_input(cache[e], all_lv[level])
    return xr_of


_CACHE = {}


def oracle(name, channel=0, n_threads=8):
    """complex128 (S, n): the literal reference path, made once per (case, channel) and read-only."""
    c = CASES[name]
    key = ("oracle", name, channel)
    if key not in _CACHE:
        x = signal(name, channel)
        if c["w0"] is not None:
            out = mc.truth(x, c["fs"], c["f"], c["w0"], bounds=[tuple(b) for b in epochs_of(name)], threads=n_threads)
        else:
            out = orc.cwt_complex(x.astype(np.float64), c["fs"], c["f"], epochs_of(name), c["gamma"], c["beta"],
                                  n_threads=n_threads)
        out.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def as_output(output, c):
    return mc.as_output(output, c)
