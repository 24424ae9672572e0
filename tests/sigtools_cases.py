"""The shapes of the operator-layer matrix (test_gpu_sigtools_matrix.py) and, in plain Python, the geometry the library
derives from them: gcwt_conv_plan_create (conv_plan.cpp), ChirpEngine::init (spectral_ops.cpp), the column-pass dispatch
of launch_fft_cols_segs (kernels.hip) and the float64 paths of ops64.hip.  test_sigtools_cases_cpu.py holds every case to
the class it is listed under; the GPU tests ask the device for the same numbers before they compare results.
No GPU, no library: integers only."""

ROW = 4096                      # kRowLen: the row pass of the two-pass FFT, P = P1 x 4096
MAX_LOG2 = 22                   # the largest float32 FFT, P1 = 1024
SEG_BATCH = 16                  # kSegBatch: chunks per launch at most
MAX_CHANNELS = 4095
ALL_P1 = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024]
MODES = ("full", "same", "valid")


def ceil_log2(v):
    return max(0, (int(v) - 1).bit_length())


# ---- float32: the convolution plan -------------------------------------------------------------------------------------
def grid_log2(n, m, fft_length):
    """ghost_amd/sigtools/convolution.py: the reference's fft_length as the plan's fft_log2."""
    log2 = max(12, ceil_log2(fft_length))
    while log2 < MAX_LOG2 and refused(n, m, 1 << log2):
        log2 += 1
    return log2


def refused(n, m, P):
    """gcwt_conv_plan_create: GCWT_ERR_UNSUPPORTED, fewer than P / 8 new samples per chunk of a chunked signal."""
    return P - (m - 1) < P // 8 and n + m - 1 > P


def conv_geometry(n, m, fft_length=None, C=1, python_layer=True):
    """What gcwt_conv_plan_create makes of (n, m, fft_log2, C).  ``python_layer``: fft_length goes through ConvPlan
    (grid_log2); else it is the C entry point's own 2^fft_log2."""
    if fft_length is None:
        P = ROW
        while P < n + 2 * (m - 1) and P < (1 << MAX_LOG2):
            P <<= 1
    else:
        P = 1 << (grid_log2(n, m, fft_length) if python_layer else max(12, ceil_log2(fft_length)))
    assert P >= m
    step = P - (m - 1)
    n_chunks = -(-(n + m - 1) // step)
    per_batch = max(1, min(SEG_BATCH, n_chunks, (2 << 30) // (8 * P * C), 65535 // C))
    n_batches = -(-n_chunks // per_batch)
    last_start = (n_chunks - 1) * step - (m - 1)             # signal index of the last chunk's sample 0
    return {"P": P, "P1": P // ROW, "step": step, "n_chunks": n_chunks, "chunks_per_batch": per_batch,
            "n_batches": n_batches, "last_batch": n_chunks - (n_batches - 1) * per_batch,
            "last_chunk_samples": min(P, n - last_start) - max(0, -last_start),      # n_valid - n_lead
            "refused": refused(n, m, P)}


# ---- float32: the chirp-z engine ---------------------------------------------------------------------------------------
def chirp_geometry(n_dft):
    """ChirpEngine::init: the circular convolution of 2 N - 1 points on P = P1 x 4096; None beyond 2^22."""
    if 2 * n_dft - 1 > (1 << MAX_LOG2):
        return None
    P = ROW
    while P < 2 * n_dft - 1:
        P <<= 1
    return {"P": P, "P1": P // ROW}


def cols_kernel(P1, sign, real_in, rows_out=None):
    """launch_fft_cols_segs as the operators call it (tables present, every segment with a real sample): the kernel of
    the column pass of P1 points.  sign -1 forward, +1 inverse."""
    rows_out = P1 if rows_out is None else rows_out
    if P1 == 256 and sign < 0 and real_in and rows_out == 129:
        return "k_fft_cols256_real2"
    if P1 in (512, 1024) and not (sign > 0 and real_in):
        lq = 2 if P1 == 1024 else 1
        if sign < 0 and real_in:
            return "k_fft_colsq_real2<%d>" % lq
        return "k_fft_colsq<%+d,complex,%d>" % (sign, lq)
    if P1 == 256:
        return "k_fft_cols256<%+d,%s>" % (sign, "real" if real_in else "complex")
    assert P1 <= 128
    return "k_fft_cols<%+d,%s>[%d]" % (sign, "real" if real_in else "complex", P1)


def conv_passes(P1):
    """The column passes one ConvPlan runs: the kernel's spectrum (complex forward), the signal (real forward) and,
    beyond one row, the inverse."""
    out = {("forward", "complex"): cols_kernel(P1, -1, False), ("forward", "real"): cols_kernel(P1, -1, True)}
    if P1 > 1:
        out[("inverse", "complex")] = cols_kernel(P1, +1, False)
    return out


def chirp_passes(P1):
    """The column passes of the chirp-z engine: complex forward (the chirp's spectrum, the modulated input -- real or
    complex input alike) and, beyond one row, the inverse."""
    out = {("forward", "complex"): cols_kernel(P1, -1, False)}
    if P1 > 1:
        out[("inverse", "complex")] = cols_kernel(P1, +1, False)
    return out


# ---- float64: ops64.hip ------------------------------------------------------------------------------------------------
def fft64_stages(lg):
    """fft64: one radix-2 stage first when lg is odd, then radix-4 stages; [(radix, lg_ns)]."""
    out, lg_ns = [], 0
    if lg & 1:
        out.append((2, 0))
        lg_ns = 1
    while lg_ns < lg:
        out.append((4, lg_ns))
        lg_ns += 2
    return out


def dft64_path(n):
    """dft_f64: a power of two is transformed directly, any other length through Bluestein on L >= 2 n - 1."""
    if n > (1 << 23):
        return None
    pow2 = n & (n - 1) == 0
    lg = ceil_log2(n if pow2 else 2 * n - 1)
    return {"path": "direct" if pow2 else "bluestein", "lg": lg, "L": 1 << lg, "radix2": bool(lg & 1)}


def conv64_path(n, m):
    """fastconv_f64: one transform of 2^lg >= n + m - 1 points up to 2^24, overlap-add chunks beyond."""
    total = n + m - 1
    if total <= (1 << 24):
        lg = ceil_log2(total)
        return {"path": "single", "lg": lg, "L": 1 << lg, "n_chunks": 1, "radix2": bool(lg & 1)}
    lg = min(24, max(22, ceil_log2(4 * m)))
    L = 1 << lg
    B = L - m + 1
    return {"path": "chunked", "lg": lg, "L": L, "n_chunks": -(-n // B), "radix2": bool(lg & 1)}


# ---- the cases ---------------------------------------------------------------------------------------------------------
# A. every P1: one convolution (C = 2, mode 'same', no fft_length)
A_CONV = [(1, 3000, 101), (2, 6000, 101), (4, 12000, 102), (8, 30000, 101), (16, 50000, 777), (32, 100000, 257),
          (64, 200000, 1000), (128, 400000, 64), (256, 700000, 1395), (512, 1500000, 2001), (1024, 3000000, 5)]
A_CONV_C = 2
# one forward and one inverse DFT of complex input per P1, 2 n - 1 in (P / 2, P]; real input at 256 and 512 as well
A_DFT = [(p1, 1500 * p1 + 7 if p1 <= 512 else 1 << 21) for p1 in ALL_P1]
A_DFT_REAL = [256, 512]
# analytic signal: (P1, n, fft_length)
A_ANALYTIC = [(8, 12001, None), (256, 300001, None), (512, 600000, 600001)]

# B. chunk geometry: fft_length 4096, m = 777 (step 3320); (n, C, n_chunks, n_batches, last batch, last chunk's samples)
B_FFT, B_M = 4096, 777
B_CHUNK = [(52344, 1, 16, 1, 16, None), (52345, 1, 17, 2, 1, 1), (100000, 3, 31, 2, 15, None)]
B_MANY = {"C": MAX_CHANNELS, "n": 1500, "m": 33}                        # one chunk, 4095 slots
B_WIDE = {"fft_length": 16384, "m": 2000, "n": 120000, "C": 2, "n_chunks": 9, "P1": 4}

# C. length edges (n, m), every defined mode, float32 and float64, real and complex kernels
C_EDGES = [(1, 1), (1, 5), (5, 1), (7, 2), (7, 7), (7, 8), (100, 1001), (1001, 100), (1000, 101), (1000, 100)]
C_SAME_PAIR = [(1000, 101), (1000, 100)]                                # the 'same' crop, odd and even m side by side
# fastconv_freq_hip (f, m, n, route): "plan" consumes the DFT as it is, "host" goes back to the time domain first.
# (4096, 4096, 10) has step = 1 and 4105 result samples: more than one chunk, so the grid is refused and doubled;
# (4096, 4096, 1) is the step = 1 plan itself: 4096 chunks of one sample each.
C_FREQ = [(4096, 1, 5000, "plan"), (4096, 2, 5000, "plan"), (4096, 4096, 10, "host"), (4096, 4096, 1, "plan"),
          (3000, 1000, 5000, "host"), (2048, 1000, 5000, "host")]

# D. float64
D_POW2 = [1 << k for k in range(13)] + [1 << 16, 1 << 17, 1 << 20]        # 2^16: between 2^16 - 1 and 2^16 + 1 below
D_BLUESTEIN = [3, 5, 6, 7, 31, 33, 2047, 2049, 65535, 65537, 1000, 100003, 3 << 21]
D_BOUNDARY_K = [5, 11, 16]
D_ANALYTIC = [(1, None), (2, None), (3, None), (1000, None), (1001, None), (1000, 1500), (1001, 2003)]
D_CONV_EXACT = [((1 << 12) - 1000 + 1, 1000), ((1 << 12) - 1000 + 2, 1000)]      # n + m - 1 = 2^12 and 2^12 + 1
D_CHUNKED = {"n": 1 << 24, "m": (1 << 20) + 3, "lg": 23, "n_chunks": 3}

# F. the grids the C entry point refuses and the Python layer doubles: (n, m, fft_length, the grid taken)
F_REFUSED = [(10000, 3700, 4096, 8192), (10000, 4096, 4096, 8192)]

# G. limits
G_DFT_MAX = 1 << 21
G_F64_MAX = 1 << 23


def freq_route(n, m, f):
    """fastconv_freq_hip (float32): 'plan' when the DFT sits on a grid the plan takes as it is."""
    ok = 4096 <= f <= (1 << MAX_LOG2) and f & (f - 1) == 0 and f >= m and (1 << grid_log2(n, m, f)) == f
    return "plan" if ok else "host"
