"""Every case of sigtools_cases.py lands in the class it is listed under: the table cannot drift away from the branches
of conv_plan.cpp, spectral_ops.cpp, kernels.hip (launch_fft_cols_segs) and ops64.hip it claims to cover.  No GPU."""
import sigtools_cases as sc


def test_every_p1_has_a_convolution():
    """A: the listed (n, m) give the listed P1 in one chunk, so the real-input forward pass, the complex forward pass
    (the kernel's spectrum) and the inverse pass each run at every column length."""
    seen = {}
    for p1, n, m in sc.A_CONV:
        g = sc.conv_geometry(n, m, None, sc.A_CONV_C)
        assert (g["P1"], g["n_chunks"], g["n_batches"], g["refused"]) == (p1, 1, 1, False), (p1, n, m, g)
        # the smallest power of two that holds n + 2 (m - 1): one size down does not
        assert g["P"] >= n + 2 * (m - 1) and (g["P"] == sc.ROW or g["P"] // 2 < n + 2 * (m - 1))
        for key, kern in sc.conv_passes(p1).items():
            seen.setdefault(key, {})[p1] = kern
    assert sorted(seen[("forward", "real")]) == sc.ALL_P1
    assert sorted(seen[("forward", "complex")]) == sc.ALL_P1
    assert sorted(seen[("inverse", "complex")]) == sc.ALL_P1[1:]         # one row: no column pass back
    # the dispatch classes of launch_fft_cols_segs, by name
    assert seen[("forward", "real")][128] == "k_fft_cols<-1,real>[128]"
    assert seen[("forward", "real")][256] == "k_fft_cols256<-1,real>"     # rows_out = 256: not the 129-row real2 kernel
    assert seen[("forward", "real")][512] == "k_fft_colsq_real2<1>"
    assert seen[("forward", "real")][1024] == "k_fft_colsq_real2<2>"
    assert seen[("forward", "complex")][256] == "k_fft_cols256<-1,complex>"
    assert seen[("forward", "complex")][512] == "k_fft_colsq<-1,complex,1>"
    assert seen[("forward", "complex")][1024] == "k_fft_colsq<-1,complex,2>"
    assert seen[("inverse", "complex")][256] == "k_fft_cols256<+1,complex>"
    assert seen[("inverse", "complex")][512] == "k_fft_colsq<+1,complex,1>"
    assert seen[("inverse", "complex")][1024] == "k_fft_colsq<+1,complex,2>"
    assert len(set(seen[("forward", "real")].values())) == 11


def test_every_p1_has_a_dft_and_the_analytic_signal_its_three():
    seen = {}
    for p1, n in sc.A_DFT:
        g = sc.chirp_geometry(n)
        assert g["P1"] == p1 and g["P"] // 2 < 2 * n - 1 <= g["P"], (p1, n, g)
        for key, kern in sc.chirp_passes(p1).items():
            seen.setdefault(key, {})[p1] = kern
    assert sorted(seen[("forward", "complex")]) == sc.ALL_P1
    assert sorted(seen[("inverse", "complex")]) == sc.ALL_P1[1:]
    assert seen[("forward", "complex")][256] == "k_fft_cols256<-1,complex>"
    assert seen[("forward", "complex")][512] == "k_fft_colsq<-1,complex,1>"
    assert set(sc.A_DFT_REAL) <= {p1 for p1, _ in sc.A_DFT}
    assert dict(sc.A_DFT)[1024] == sc.G_DFT_MAX
    for p1, n, f in sc.A_ANALYTIC:
        assert sc.chirp_geometry(n if f is None else f)["P1"] == p1, (p1, n, f)
    assert [p1 for p1, _, _ in sc.A_ANALYTIC] == [8, 256, 512]


def test_chunk_geometry_cases():
    """B: batches after the first, a ragged last batch, a last chunk of one real sample, C > 1 with two batches, the
    channel cap, chunks beyond one row."""
    step = sc.B_FFT - (sc.B_M - 1)
    assert step == 3320
    for n, C, n_chunks, n_batches, last_batch, last_samples in sc.B_CHUNK:
        g = sc.conv_geometry(n, sc.B_M, sc.B_FFT, C)
        assert (g["P"], g["P1"], g["step"]) == (4096, 1, step)
        assert (g["n_chunks"], g["n_batches"], g["last_batch"]) == (n_chunks, n_batches, last_batch), (n, C, g)
        assert g["chunks_per_batch"] == 16 and not g["refused"]
        if last_samples is not None:
            assert g["last_chunk_samples"] == last_samples
    got = [sc.conv_geometry(n, sc.B_M, sc.B_FFT, C) for n, C, *_ in sc.B_CHUNK]
    assert got[0]["n_batches"] == 1 and (got[0]["n_chunks"] * step == 52344 + sc.B_M - 1)      # exactly full
    assert got[1]["n_batches"] > 1 and got[1]["last_batch"] == 1 and got[1]["last_chunk_samples"] == 1
    assert got[2]["n_batches"] > 1 and 1 < got[2]["last_batch"] < 16 and sc.B_CHUNK[2][1] > 1    # ragged, C > 1
    g = sc.conv_geometry(sc.B_MANY["n"], sc.B_MANY["m"], None, sc.B_MANY["C"])
    assert (g["P1"], g["n_chunks"], g["chunks_per_batch"]) == (1, 1, 1) and sc.B_MANY["C"] == sc.MAX_CHANNELS == 4095
    w = sc.B_WIDE
    g = sc.conv_geometry(w["n"], w["m"], w["fft_length"], w["C"])
    assert (g["P1"], g["n_chunks"], g["n_batches"]) == (w["P1"], w["n_chunks"], 1) and g["P"] == 16384


def test_length_edges_cover_their_classes():
    nm = sc.C_EDGES
    assert (1, 1) in nm
    assert any(m == 1 and n > 1 for n, m in nm)                       # step = P, no history
    assert any(m == 2 for n, m in nm)
    assert any(n == 1 and m > 1 for n, m in nm)
    assert any(n < m and n > 1 for n, m in nm)                        # 'same' and 'full' only
    assert any(n == m and n > 1 for n, m in nm)                       # 'valid': one sample
    assert sum(n > m > 1 for n, m in nm) >= 3
    (n0, m0), (n1, m1) = sc.C_SAME_PAIR
    assert n0 == n1 and m0 % 2 == 1 and m1 % 2 == 0 and m0 - m1 == 1
    assert (n0 + m0 - 1 - n0) // 2 == (n1 + m1 - 1 - n1) // 2 + 1 == 50           # the crops differ by one sample
    assert set(sc.C_SAME_PAIR) <= set(nm)
    for n, m in nm:
        g = sc.conv_geometry(n, m)
        assert (g["P1"], g["n_chunks"]) == (1, 1)
    for f, m, n, route in sc.C_FREQ:
        assert sc.freq_route(n, m, f) == route, (f, m, n)
        if route == "plan":
            g = sc.conv_geometry(n, m, f)
            assert g["P"] == f and g["step"] == f - m + 1 and not g["refused"]
    assert {(f, m) for f, m, _, _ in sc.C_FREQ} >= {(4096, 1), (4096, 2), (4096, 4096)}
    assert {f for f, _, _, r in sc.C_FREQ if r == "host"} >= {3000, 2048}
    one = sc.conv_geometry(1, 4096, 4096)
    assert (one["step"], one["n_chunks"], one["n_batches"]) == (1, 4096, 256)
    assert sc.conv_geometry(10, 4096, 4096, python_layer=False)["refused"]


def test_float64_paths():
    """D: log2 L from 0 to 12 directly (the radix-2 stage at every odd one), both Bluestein boundaries, lg = 23 chunked."""
    direct = {sc.dft64_path(n)["lg"]: sc.dft64_path(n) for n in sc.D_POW2}
    assert all(p["path"] == "direct" for p in direct.values())
    assert sorted(direct) == list(range(13)) + [16, 17, 20]
    for lg, p in direct.items():
        st = sc.fft64_stages(lg)
        assert p["radix2"] == (lg % 2 == 1) == (bool(st) and st[0] == (2, 0))
        assert sum(1 if r == 2 else 2 for r, _ in st) == lg
        assert [s for _, s in st] == ([0] if lg & 1 else []) + list(range(lg & 1, lg, 2))
    assert sc.fft64_stages(0) == [] and sc.fft64_stages(1) == [(2, 0)] and sc.fft64_stages(3) == [(2, 0), (4, 1)]
    blue = {n: sc.dft64_path(n) for n in sc.D_BLUESTEIN}
    assert all(p["path"] == "bluestein" and p["L"] >= 2 * n - 1 > p["L"] // 2 for n, p in blue.items())
    for k in sc.D_BOUNDARY_K:
        below, at, above = (1 << k) - 1, 1 << k, (1 << k) + 1
        assert below in blue and above in blue and at in sc.D_POW2
        assert sc.dft64_path(at)["path"] == "direct"
        assert blue[below]["lg"] == k + 1 and blue[above]["lg"] == k + 2      # the two sides sit on different grids
    assert {blue[n]["radix2"] for n in blue} == {True, False}
    assert blue[3 << 21]["lg"] == 24 and blue[3]["lg"] == 3 and blue[100003]["lg"] == 18
    for n, f in sc.D_ANALYTIC:
        assert sc.dft64_path(n if f is None else f) is not None
    (na, ma), (nb, mb) = sc.D_CONV_EXACT
    a, b = sc.conv64_path(na, ma), sc.conv64_path(nb, mb)
    assert na + ma - 1 == 1 << 12 and nb + mb - 1 == (1 << 12) + 1
    assert (a["path"], a["lg"], b["path"], b["lg"]) == ("single", 12, "single", 13)
    c = sc.D_CHUNKED
    p = sc.conv64_path(c["n"], c["m"])
    assert (p["path"], p["lg"], p["n_chunks"], p["radix2"]) == ("chunked", c["lg"], c["n_chunks"], True)
    assert sc.conv64_path((1 << 24) + 300001, 1395)["lg"] == 22               # what test_gpu_sigtools.py runs


def test_refused_grids_and_limits():
    for n, m, f, taken in sc.F_REFUSED:
        assert sc.conv_geometry(n, m, f, python_layer=False)["refused"]
        g = sc.conv_geometry(n, m, f)
        assert g["P"] == taken and not g["refused"] and g["n_chunks"] > 1
        assert sc.freq_route(n, m, f) == "host"
    assert sc.conv_geometry(10000, 4096, 4096, python_layer=False)["step"] == 1
    # a kernel over 7/8 of 2^22 taps on a longer signal stays refused: nothing larger to take
    assert sc.conv_geometry(1 << 23, (7 << 19) + 2, 1 << 22)["refused"]
    assert sc.chirp_geometry(sc.G_DFT_MAX)["P1"] == 1024 and sc.chirp_geometry(sc.G_DFT_MAX + 1) is None
    assert sc.dft64_path(sc.G_F64_MAX)["lg"] == 23 and sc.dft64_path(sc.G_F64_MAX + 1) is None
    assert sc.grid_log2(100, 10, 1) == 12 and sc.grid_log2(100, 10, 1 << 22) == 22
