"""Thin Python handle on a libghostcwt plan (host side of the C ABI).

``CwtPlan`` is what ``ContinuousWaveletTransform.transform`` drives; bench.py
and the tests use it directly for device-resident runs.  All arithmetic happens
in the HIP library.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib, check

__all__ = ["CwtPlan", "DeviceBuffer", "DeviceResult", "CoherenceResult", "coherence", "coherence_pairs", "CouplingResult",
           "coupling", "coupling_rows", "CouplingSurrogatesResult", "coupling_surrogates", "surrogate_shifts", "TriggeredResult", "triggered", "trigger_columns", "BandpassResult",
           "bandpass", "band_rows", "band_weights", "RidgeResult", "ridge", "ridge_weights", "trace_stats", "trace_runs", "trace_order", "trace_median_mad", "smooth_taps", "segments_of",
           "trace_smooth", "event_filter", "set_option",
           "device_count", "device_name", "device_memory"]


def set_option(name, value=None):
    """Test / measurement switch of the library (include/ghostcwt_debug.h: gcwt_debug_set_option), read by
    plans created afterwards; ``value=None`` restores the default."""
    check(lib.gcwt_debug_set_option(name.encode(), 0 if value is None else int(value), 1 if value is None else 0))


def device_count():
    n = C.c_int(0)
    rc = lib.gcwt_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def device_name(device=0):
    buf = C.create_string_buffer(256)
    check(lib.gcwt_device_name(device, buf, 256))
    return buf.value.decode()


def device_memory():
    """(free, total) bytes of the current device."""
    free, total = C.c_size_t(0), C.c_size_t(0)
    check(lib.gcwt_device_memory(C.byref(free), C.byref(total)))
    return free.value, total.value


class DeviceBuffer:
    """hipMalloc'd bytes owned by Python."""

    def __init__(self, nbytes):
        self.ptr = C.c_void_p()
        self.nbytes = int(nbytes)
        check(lib.gcwt_device_malloc(C.byref(self.ptr), self.nbytes))

    def upload(self, array, offset_bytes=0):
        a = np.ascontiguousarray(array)
        assert offset_bytes + a.nbytes <= self.nbytes
        dst = C.c_void_p(self.ptr.value + offset_bytes)
        check(lib.gcwt_memcpy_h2d(dst, a.ctypes.data_as(C.c_void_p), a.nbytes))

    def download(self, shape, dtype, offset_bytes=0):
        out = np.empty(shape, dtype=dtype)
        assert offset_bytes + out.nbytes <= self.nbytes
        src = C.c_void_p(self.ptr.value + offset_bytes)
        check(lib.gcwt_memcpy_d2h(out.ctypes.data_as(C.c_void_p), src, out.nbytes))
        return out

    def zero(self):
        check(lib.gcwt_device_memset(self.ptr, 0, self.nbytes))

    def free(self):
        if self.ptr:
            lib.gcwt_device_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceResult:
    """A transform's result left on the device: ``shape`` (C, S, N) rows of float32 (complex64 for complex
    output), ``pitch`` samples apart.  ``to_host`` brings over the whole result or any (scale, sample) range
    of it -- straight into page-locked memory at the link's rate (ghost_amd.hostmem), float64 widened on the
    device -- and ``buffer.ptr`` is the handle for whoever keeps working on the device."""

    def __init__(self, buffer, shape, pitch, complex_):
        self.buffer, self.shape, self.pitch, self.is_complex = buffer, tuple(int(v) for v in shape), int(pitch), bool(complex_)

    @property
    def nbytes(self):
        return self.shape[0] * self.shape[1] * self.pitch * (8 if self.is_complex else 4)

    def to_host(self, dtype=None, scales=None, start=0, stop=None):
        """ndarray (C, S', n): scales ``scales`` (slice or None = all), samples [start, stop) of every channel.
        dtype: float32 / float64 (complex64 / complex128 for complex results); default the device's."""
        from . import hostmem
        c, s, n = self.shape
        k = 2 if self.is_complex else 1
        narrow = np.complex64 if self.is_complex else np.float32
        wide = np.complex128 if self.is_complex else np.float64
        dtype = np.dtype(narrow if dtype is None else dtype)
        if dtype not in (np.dtype(narrow), np.dtype(wide)):
            raise ValueError("dtype must be %s or %s" % (np.dtype(narrow), np.dtype(wide)))
        if isinstance(scales, (int, np.integer)):
            scales = slice(int(scales), int(scales) + 1) if scales != -1 else slice(-1, None)
        sl = range(s)[slice(None) if scales is None else scales]
        if sl.step != 1 and len(sl) > 1:
            raise ValueError("scales must be a contiguous range")
        stop = n if stop is None else min(int(stop), n)
        start = max(0, int(start))
        cols = max(0, stop - start)
        out_shape = (c, len(sl), cols)
        out = hostmem.empty(out_shape, dtype)
        pinned = out is not None
        if not pinned:
            out = np.empty(out_shape, dtype=dtype)
        if out.size == 0:
            return out
        flags = (_lib.OUT_F64 if dtype == np.dtype(wide) else 0) | (_lib.HOST_PINNED if pinned else 0)
        esz = 4 * k
        if len(sl) == s:                       # all scales: the channels' rows follow each other
            groups = [(0, c * s, out.reshape(c * s, cols))]
        else:
            groups = [(ch * s + sl.start, len(sl), out[ch]) for ch in range(c)]
        for row0, n_rows, dst in groups:
            src = C.c_void_p(self.buffer.ptr.value + (row0 * self.pitch + start) * esz)
            check(lib.gcwt_rows_to_host(src, self.pitch * k, n_rows, cols * k, dst.ctypes.data_as(C.c_void_p),
                                        cols * k, flags))
        return out

    def free(self):
        if self.buffer is not None:
            self.buffer.free()
            self.buffer = None


_OUT_DTYPE = {_lib.OUT_AMPLITUDE: np.float32, _lib.OUT_POWER: np.float32,
              _lib.OUT_COMPLEX: np.complex64}
_OUT_MODES = {"amplitude": _lib.OUT_AMPLITUDE, "power": _lib.OUT_POWER,
              "complex": _lib.OUT_COMPLEX}


def output_stride_value(stride):
    """The output stride K as an int: an integer >= 1 (numpy integers too); anything else -- bool, a float, K < 1 --
    raises ValueError."""
    if isinstance(stride, (bool, np.bool_)) or not isinstance(stride, (int, np.integer)):
        raise ValueError("output_stride must be an integer >= 1, not %r" % (stride,))
    if int(stride) < 1:
        raise ValueError("output_stride must be an integer >= 1, not %d" % int(stride))
    return int(stride)


def coherence_pairs(pairs, seed, n_channels):
    """The channel pairs of a coherence() call as a (P, 2) int32 array.  ``pairs=None, seed=None``: all (a, b), a < b, in
    lexicographic order; ``seed=c``: (c, k) for every k != c, k ascending; else ``pairs``: (P, 2) integers, a != b, both
    in [0, n_channels).  Anything else -- floats, bools, a == b, an index out of range, ``pairs`` and ``seed`` together
    -- raises ValueError."""
    n = int(n_channels)
    if n < 2:
        raise ValueError("coherence needs at least 2 channels, not %d" % n)
    if pairs is not None and seed is not None:
        raise ValueError("'pairs' and 'seed' cannot both be used")
    if pairs is None and seed is None:
        a, b = np.triu_indices(n, 1)
        return np.ascontiguousarray(np.stack([a, b], axis=1), dtype=np.int32)
    if pairs is None:
        if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)):
            raise ValueError("'seed' must be a channel index (an integer), not %r" % (seed,))
        if not 0 <= int(seed) < n:
            raise ValueError("'seed' %d is not a channel of the result (0 .. %d)" % (int(seed), n - 1))
        others = np.array([k for k in range(n) if k != int(seed)], dtype=np.int32)
        return np.ascontiguousarray(np.stack([np.full_like(others, int(seed)), others], axis=1))
    arr = np.asarray(pairs)
    if arr.dtype == np.bool_ or not np.issubdtype(arr.dtype, np.integer):
        raise ValueError("'pairs' must be an array of integer channel indices, not %s" % arr.dtype)
    if arr.ndim != 2 or arr.shape[1] != 2 or arr.shape[0] < 1:
        raise ValueError("'pairs' must have shape (P, 2), P >= 1, not %r" % (arr.shape,))
    if arr.min() < 0 or arr.max() >= n:
        raise ValueError("'pairs' names a channel outside 0 .. %d" % (n - 1))
    if np.any(arr[:, 0] == arr[:, 1]):
        raise ValueError("'pairs' holds a channel paired with itself")
    return np.ascontiguousarray(arr, dtype=np.int32)


def _is_number(v):
    """A real number, Python's or numpy's, and no bool."""
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))


def _ptr(arr, ctype):
    """``arr`` as the C entries take an array of ``ctype``; None stays None."""
    return None if arr is None else arr.ctypes.data_as(C.POINTER(ctype))


def bin_window(window):
    """The bin width as an int: an integer >= 2 (numpy integers too); anything else raises ValueError."""
    if isinstance(window, (bool, np.bool_)) or not isinstance(window, (int, np.integer)):
        raise ValueError("window must be an integer >= 2 (columns per bin), not %r" % (window,))
    if int(window) < 2:
        raise ValueError("window must be an integer >= 2 (columns per bin), not %d" % int(window))
    return int(window)


coherence_window = bin_window                               # (the name it had while coherence() was its only user)


class _RowOpResult:
    """What an operator on the rows of a resident result left on the device: planes of float32 / complex64 rows, ``pitch``
    elements apart, one after the other in one DeviceBuffer.  A subclass's ``_planes()`` says which: ((name, dtype,
    leading shape), ...) in buffer order, and how many elements of a row are live."""

    def _plane_bytes(self):
        return [(name, int(np.prod(lead, dtype=np.int64)) * self.pitch * np.dtype(dtype).itemsize)
                for name, dtype, lead in self._planes()[0]]

    def _offsets(self):
        """name -> the plane's first byte."""
        offsets, end = {}, 0
        for name, nbytes in self._plane_bytes():
            offsets[name] = end
            end += nbytes
        return offsets

    @property
    def nbytes(self):
        return sum(nbytes for _, nbytes in self._plane_bytes())

    def to_host(self):
        """name -> dense ndarray, for every plane."""
        planes, live = self._planes()
        offsets = self._offsets()
        return {name: np.ascontiguousarray(self.buffer.download(tuple(lead) + (self.pitch,), dtype, offsets[name])[..., :live])
                for name, dtype, lead in planes}

    def free(self):
        if self.buffer is not None:
            self.buffer.free()
            self.buffer = None


def _pitch(n):
    return (n + 31) & ~31                                   # rows start on 128-byte lines


def _resident_complex(result, what, sharded_reason):
    """The shape (C, S, N) of ``result`` if operator ``what`` can work on it: a complex DeviceResult that still has its
    buffer."""
    if not isinstance(result, DeviceResult):
        raise ValueError("%s() takes a DeviceResult on one device (%s)" % (what, sharded_reason))
    if result.buffer is None:
        raise ValueError("the result has been freed")
    if not result.is_complex:
        raise ValueError("%s() needs complex coefficients (output='complex')" % what)
    return result.shape


def _run_into(res, what, sizes, advice, call):
    """Gives ``res`` its buffer -- MemoryError, in the operator's words, where the device has not that much free -- and
    runs ``call(ptr)``, ptr: plane name -> c_void_p; a call that fails takes the buffer with it.  -> res."""
    nbytes = res.nbytes
    free, _ = device_memory()
    if nbytes > free:
        raise MemoryError("%s() needs %d bytes on the device for its outputs (%s) and %d are free: %s"
                          % (what, nbytes, sizes, free, advice))
    res.buffer = buf = DeviceBuffer(nbytes)
    ptr = {name: C.c_void_p(buf.ptr.value + off) for name, off in res._offsets().items()}
    try:
        call(ptr)
    except Exception:
        res.free()
        raise
    return res


class CoherenceResult(_RowOpResult):
    """What coherence() left on the device: ``coherence`` (P, S, B) float32, ``cross`` (P, S, B) complex64 and ``power``
    (C, S, B) float32 in one DeviceBuffer, rows ``pitch`` elements apart; ``pairs`` (P, 2); ``window``; ``counts`` (B,):
    the columns of each bin.  ``to_host()`` brings the three over."""

    def __init__(self, buffer, pairs, n_channels, n_scales, n_bins, pitch, window, counts):
        self.buffer, self.pairs, self.pitch, self.window, self.counts = buffer, pairs, int(pitch), int(window), counts
        self.n_pairs, self.n_channels, self.n_scales, self.n_bins = len(pairs), int(n_channels), int(n_scales), int(n_bins)

    def _planes(self):
        p, c, s = self.n_pairs, self.n_channels, self.n_scales
        return (("cross", np.complex64, (p, s)), ("coherence", np.float32, (p, s)), ("power", np.float32, (c, s))), self.n_bins


def _bin_counts(n, window, n_bins):
    return np.minimum(window, n - np.arange(n_bins, dtype=np.int64) * window)


def coherence(result, pairs, window):
    """Binned cross-spectra of channel pairs of a complex DeviceResult, computed where it lies (gcwt_coherence: bins of
    ``window`` columns; include/ghostcwt.h has the definition).  ``pairs``: (P, 2) as coherence_pairs returns them.  The
    result itself is only read.  -> CoherenceResult."""
    window = bin_window(window)
    c, s, n = _resident_complex(result, "coherence", "the channels of a result sharded over several GPUs cannot be paired")
    pairs = coherence_pairs(pairs, None, c)
    n_bins = -(-n // window)
    p = len(pairs)
    res = CoherenceResult(None, pairs, c, s, n_bins, _pitch(n_bins), window, _bin_counts(n, window, n_bins))
    return _run_into(
        res, "coherence", "%d pairs, %d channels, %d scales, %d bins" % (p, c, s, n_bins), "fewer pairs or a wider window",
        lambda ptr: check(lib.gcwt_coherence(result.buffer.ptr, result.pitch, c, s, n,
                                             _ptr(pairs, C.c_int32), p, window, ptr["power"],
                                             ptr["cross"], ptr["coherence"], res.pitch)))


def coupling_rows(limits, frequencies, what):
    """The rows of a coupling() band as (first, count): those whose frequency lies in the closed interval ``limits`` =
    (f_lo, f_hi) in Hz, f_lo <= f_hi.  ``frequencies`` is monotonic (descending for the default grid, ascending for
    ``freqs=``), so the rows are one contiguous run.  ``what`` ('phase', 'amplitude') names the band in the ValueError
    that anything else raises: not two finite numbers, f_lo > f_hi, no row inside."""
    try:
        ok = not isinstance(limits, (str, bytes)) and len(limits) == 2 and not any(
            not _is_number(v) for v in limits)
    except TypeError:
        ok = False
    if not ok or not all(np.isfinite(float(v)) for v in limits):
        raise ValueError("'%s' must be (f_lo, f_hi) in Hz, two finite numbers, not %r" % (what, limits))
    lo, hi = float(limits[0]), float(limits[1])
    if lo > hi:
        raise ValueError("'%s' must be (f_lo, f_hi) with f_lo <= f_hi, not %r" % (what, limits))
    f = np.asarray(frequencies, dtype=np.float64).ravel()
    rows = np.flatnonzero((f >= lo) & (f <= hi))
    if rows.size == 0:
        raise ValueError("'%s': no row of the transform has its frequency in [%g, %g] Hz (the rows span %g .. %g Hz)"
                         % (what, lo, hi, f.min() if f.size else np.nan, f.max() if f.size else np.nan))
    if rows[-1] - rows[0] + 1 != rows.size:
        raise ValueError("'%s': the frequencies are not monotonic" % what)
    return int(rows[0]), int(rows.size)


class CouplingResult(_RowOpResult):
    """What coupling() left on the device: ``vector`` (C, P, A, B) complex64, ``mvl`` (C, P, A, B) float32 and
    ``amplitude`` (C, A, B) float32 in one DeviceBuffer, rows ``pitch`` elements apart; ``phase_rows`` and ``amp_rows``:
    (first, count); ``window``; ``counts`` (B,): the columns of each bin.  ``to_host()`` brings the three over."""

    def __init__(self, buffer, n_channels, phase_rows, amp_rows, n_bins, pitch, window, counts):
        self.buffer, self.pitch, self.window, self.counts = buffer, int(pitch), int(window), counts
        self.phase_rows, self.amp_rows = tuple(phase_rows), tuple(amp_rows)
        self.n_channels, self.n_phase, self.n_amp, self.n_bins = int(n_channels), int(phase_rows[1]), int(amp_rows[1]), int(n_bins)

    def _planes(self):
        c, p, a = self.n_channels, self.n_phase, self.n_amp
        return (("vector", np.complex64, (c, p, a)), ("mvl", np.float32, (c, p, a)), ("amplitude", np.float32, (c, a))), self.n_bins


def _row_range(rows, n_scales, what):
    try:
        first, count = rows
        ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in (first, count))
    except (TypeError, ValueError):
        ok = False
    if not ok or first < 0 or count < 1 or first + count > n_scales:
        raise ValueError("%s must be (first, count), a non-empty run of the result's %d rows, not %r" % (what, n_scales, rows))
    return int(first), int(count)


def coupling(result, phase_rows, amp_rows, window):
    """Binned phase-amplitude coupling inside every channel of a complex DeviceResult, computed where it lies
    (gcwt_coupling: bins of ``window`` columns; include/ghostcwt.h has the definition).  ``phase_rows``, ``amp_rows``:
    (first, count) as coupling_rows returns them; they may overlap.  The result itself is only read.  -> CouplingResult."""
    window = bin_window(window)
    c, s, n = _resident_complex(result, "coupling", "a result sharded over several GPUs is not supported")
    phase_rows = _row_range(phase_rows, s, "phase_rows")
    amp_rows = _row_range(amp_rows, s, "amp_rows")
    n_bins = -(-n // window)
    res = CouplingResult(None, c, phase_rows, amp_rows, n_bins, _pitch(n_bins), window, _bin_counts(n, window, n_bins))
    return _run_into(
        res, "coupling", "%d channels, %d x %d rows, %d bins" % (c, phase_rows[1], amp_rows[1], n_bins),
        "narrower bands or a wider window",
        lambda ptr: check(lib.gcwt_coupling(result.buffer.ptr, result.pitch, c, s, n, phase_rows[0], phase_rows[1],
                                            amp_rows[0], amp_rows[1], window, ptr["vector"], ptr["mvl"], ptr["amplitude"],
                                            res.pitch)))


def surrogate_shifts(k, window, min_cols, seed):
    """The shift list of a coupling_surrogates() call: ``np.random.default_rng(seed).integers(min_cols, window - min_cols
    + 1, size=k)`` as int64 -- ``k`` shifts in columns, each at least ``min_cols`` away from 0 and from ``window`` (a
    shift below about one period of the phase rhythm leaves the coupling in place).  ValueError unless ``k`` is an int
    in 2 .. 4096, ``min_cols`` an int >= 1 and ``window >= 2 min_cols + 1``."""
    window = bin_window(window)
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 2 <= int(k) <= 4096:
        raise ValueError("the number of surrogates must be an integer in 2 .. 4096, not %r" % (k,))
    if isinstance(min_cols, (bool, np.bool_)) or not isinstance(min_cols, (int, np.integer)) or int(min_cols) < 1:
        raise ValueError("the smallest shift must be an integer number of columns >= 1, not %r" % (min_cols,))
    if window < 2 * int(min_cols) + 1:
        raise ValueError("window = %d columns leaves no shift at least %d columns away from both ends of a bin: it must "
                         "be at least 2 x %d + 1" % (window, int(min_cols), int(min_cols)))
    return np.random.default_rng(seed).integers(int(min_cols), window - int(min_cols) + 1, size=int(k)).astype(np.int64)


class CouplingSurrogatesResult(_RowOpResult):
    """What coupling_surrogates() left on the device: ``mean`` and ``sd`` (C, P, A, B) float32, ``count_ge`` (C, P, A, B)
    int32 and, when kept, ``surrogates`` (K, C, P, A, B) float32 in one DeviceBuffer, rows ``pitch`` elements apart;
    ``shifts`` (K,) int64; ``phase_rows`` and ``amp_rows``: (first, count); ``window``; ``counts`` (B,): the columns of
    each bin.  ``to_host()`` brings the planes over."""

    def __init__(self, buffer, n_channels, phase_rows, amp_rows, n_bins, pitch, window, counts, shifts, keep):
        self.buffer, self.pitch, self.window, self.counts = buffer, int(pitch), int(window), counts
        self.phase_rows, self.amp_rows, self.shifts, self.keep = tuple(phase_rows), tuple(amp_rows), shifts, bool(keep)
        self.n_channels, self.n_phase, self.n_amp, self.n_bins = int(n_channels), int(phase_rows[1]), int(amp_rows[1]), int(n_bins)

    def _planes(self):
        lead = (self.n_channels, self.n_phase, self.n_amp)
        planes = (("mean", np.float32, lead), ("sd", np.float32, lead), ("count_ge", np.int32, lead))
        if self.keep:
            planes += (("surrogates", np.float32, (len(self.shifts),) + lead),)
        return planes, self.n_bins


def coupling_surrogates(result, phase_rows, amp_rows, window, shifts, keep=False):
    """Shift-surrogate statistics of coupling()'s mvl, computed where the result lies (gcwt_coupling_surrogates;
    include/ghostcwt.h has the definition): for every shift of ``shifts`` (1-D integers, 2 .. 4096 of them, each in [0,
    window) columns; surrogate_shifts() draws such a list) the amplitude row is moved circularly inside each bin and the
    mvl made again.  ``window`` is at most _lib.COUPLING_SURROGATES_MAX_WINDOW columns.  ``keep``: every surrogate mvl
    stays too.  The result itself is only read.  -> CouplingSurrogatesResult."""
    window = bin_window(window)
    c, s, n = _resident_complex(result, "coupling_surrogates", "a result sharded over several GPUs is not supported")
    phase_rows = _row_range(phase_rows, s, "phase_rows")
    amp_rows = _row_range(amp_rows, s, "amp_rows")
    if window > _lib.COUPLING_SURROGATES_MAX_WINDOW:
        raise ValueError("window = %d columns is above the largest the surrogates can take, %d (a bin is held in the LDS of "
                         "one compute unit): a shorter window or an output_stride" % (window, _lib.COUPLING_SURROGATES_MAX_WINDOW))
    arr = np.asarray(shifts)
    if arr.dtype == np.bool_ or not np.issubdtype(arr.dtype, np.integer) or arr.ndim != 1:
        raise ValueError("shifts must be a 1-D array of integer shifts in columns, not %s of shape %r" % (arr.dtype, arr.shape))
    if not 2 <= arr.size <= 4096:
        raise ValueError("shifts must hold 2 .. 4096 shifts, not %d" % arr.size)
    arr = np.ascontiguousarray(arr, dtype=np.int64)
    bad = np.flatnonzero((arr < 0) | (arr >= window))
    if bad.size:
        raise ValueError("shifts[%d] = %d is outside [0, window = %d)" % (bad[0], arr[bad[0]], window))
    n_bins = -(-n // window)
    res = CouplingSurrogatesResult(None, c, phase_rows, amp_rows, n_bins, _pitch(n_bins), window,
                                   _bin_counts(n, window, n_bins), arr, keep)
    return _run_into(
        res, "coupling_surrogates", "%d channels, %d x %d rows, %d bins%s"
        % (c, phase_rows[1], amp_rows[1], n_bins, ", %d surrogates kept" % arr.size if keep else ""),
        "narrower bands, a wider window or keep=False",
        lambda ptr: check(lib.gcwt_coupling_surrogates(result.buffer.ptr, result.pitch, c, s, n, phase_rows[0], phase_rows[1],
                                                       amp_rows[0], amp_rows[1], window,
                                                       _ptr(arr, C.c_int64), arr.size, ptr["mean"], ptr["sd"],
                                                       ptr["count_ge"], ptr.get("surrogates"), res.pitch)))


def _seconds(value, what):
    if not _is_number(value) or not np.isfinite(float(value)) or float(value) < 0:
        raise ValueError("'%s' must be a finite number of seconds >= 0, not %r" % (what, value))
    return float(value)


def _trigger_scan(events, time, fs, stride, before, after, n_cols):
    """trigger_columns plus why events were dropped: {"gap": not within half a column period of any column, "edge": the
    window leaves the columns, "splice": the window would join two epochs} -> counts."""
    before, after = _seconds(before, "before"), _seconds(after, "after")
    try:
        ev = np.asarray(events)
        ok = ev.ndim == 1 and ev.dtype != np.bool_ and (np.issubdtype(ev.dtype, np.integer) or np.issubdtype(ev.dtype, np.floating))
    except Exception:
        ok = False
    if not ok:
        raise ValueError("'events' must be a 1-D array of event times in seconds (finite numbers), not %r"
                         % (getattr(events, "shape", None) if hasattr(events, "dtype") else events,))
    ev = ev.astype(np.float64)
    if not np.all(np.isfinite(ev)):
        raise ValueError("'events' must be finite: entry %d is %r" % (int(np.flatnonzero(~np.isfinite(ev))[0]),
                                                                      float(ev[~np.isfinite(ev)][0])))
    period = float(stride) / float(fs)                      # seconds per column
    nb, na = int(round(before / period)), int(round(after / period))
    if time is None:
        col = np.clip(np.rint(ev / period), -1, 2.0 ** 62).astype(np.int64)      # (-1: before the first sample)
        near = col >= 0 if n_cols is None else (col >= 0) & (col < n_cols)
        t = None
    else:
        t = np.asarray(time, dtype=np.float64).ravel()
        n_cols = t.size if n_cols is None else min(int(n_cols), t.size)
        t = t[:n_cols]
        if n_cols == 0:
            raise ValueError("'time' holds no column")
        hi = np.clip(np.searchsorted(t, ev), 0, n_cols - 1)
        lo = np.clip(hi - 1, 0, None)
        col = np.where(np.abs(t[lo] - ev) <= np.abs(t[hi] - ev), lo, hi).astype(np.int64)
        near = np.abs(t[col] - ev) <= 0.5 * period
    inside = near & (col - nb >= 0) & (True if n_cols is None else col + na < n_cols)
    whole = inside.copy()
    if t is not None and inside.any():
        span = t[np.where(inside, col + na, 0)] - t[np.where(inside, col - nb, 0)]
        whole &= np.abs(span - (nb + na) * period) <= 0.5 / float(fs)
    reasons = {"gap": int(np.count_nonzero(~near)), "edge": int(np.count_nonzero(near & ~inside)),
               "splice": int(np.count_nonzero(inside & ~whole))}
    return np.ascontiguousarray(col[whole], dtype=np.int64), whole, nb, na, reasons


def trigger_columns(events, time, fs, stride, before, after, n_cols=None):
    """Event times -> the columns triggered() gathers around.  ``events``: 1-D, seconds on the clock of ``time`` (the
    times of the result's columns, ``ContinuousWaveletTransform.time``; None: seconds from the first sample, column j at
    j stride / fs -- ``n_cols`` then bounds the columns).  ``before``, ``after``: seconds >= 0, nb = round(before fs /
    stride) columns and na likewise.  An event maps to its nearest column and is dropped when that column is more than
    half a column period away (the event lies in a gap between epochs or outside the recording), when its window leaves
    [0, n_cols), or when time[col + na] - time[col - nb] differs from (nb + na) stride / fs by more than half a sample
    period (the window would splice two epochs).  -> (cols int64: the surviving events' columns in the order given,
    used: bool mask over ``events``, nb, na).  ValueError naming 'events', 'before' or 'after' for anything that is not a
    1-D array of finite numbers or a finite number >= 0."""
    return _trigger_scan(events, time, fs, stride, before, after, n_cols)[:4]


class TriggeredResult(_RowOpResult):
    """What triggered() left on the device, each (C, R, L) with rows ``pitch`` elements apart in one DeviceBuffer:
    ``evoked`` and ``vector`` complex64, ``amplitude``, ``power`` and ``itpc`` float32; ``rows``: (first, count);
    ``n_before``, ``n_after`` columns, L = n_before + n_after + 1 lags; ``n_events``.  ``to_host()`` brings the five over."""

    def __init__(self, buffer, n_channels, rows, n_before, n_after, pitch, n_events):
        self.buffer, self.pitch, self.rows = buffer, int(pitch), tuple(rows)
        self.n_channels, self.n_rows, self.n_events = int(n_channels), int(rows[1]), int(n_events)
        self.n_before, self.n_after, self.n_lags = int(n_before), int(n_after), int(n_before) + int(n_after) + 1

    def _planes(self):
        lead = (self.n_channels, self.n_rows)
        return (("evoked", np.complex64, lead), ("vector", np.complex64, lead), ("amplitude", np.float32, lead),
                ("power", np.float32, lead), ("itpc", np.float32, lead)), self.n_lags


def _columns(value, what):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or int(value) < 0:
        raise ValueError("%s must be an integer number of columns >= 0, not %r" % (what, value))
    return int(value)


def triggered(result, cols, nb, na, rows=None):
    """Event-locked averages of the rows of a complex DeviceResult, computed where it lies (gcwt_triggered;
    include/ghostcwt.h has the definition): around every event column of ``cols`` (1-D integers, in this order; the order
    is part of the definition of the float32 sums) the window of ``nb`` columns before and ``na`` after, which must lie
    inside the result for every event -- trigger_columns() makes such a list from event times.  ``rows``: (first, count),
    default all rows.  The result itself is only read.  -> TriggeredResult."""
    c, s, n = _resident_complex(result, "triggered", "a result sharded over several GPUs is not supported")
    nb, na = _columns(nb, "nb"), _columns(na, "na")
    rows = _row_range((0, s) if rows is None else rows, s, "rows")
    arr = np.asarray(cols)
    if arr.dtype == np.bool_ or not np.issubdtype(arr.dtype, np.integer) or arr.ndim != 1:
        raise ValueError("cols must be a 1-D array of integer event columns, not %s of shape %r" % (arr.dtype, arr.shape))
    if not 1 <= arr.size <= 1 << 24:
        raise ValueError("cols must hold 1 .. 2^24 event columns, not %d" % arr.size)
    n_lags = nb + na + 1
    if n_lags > n:
        raise ValueError("the window of nb + na + 1 = %d columns is longer than the result's %d" % (n_lags, n))
    arr = np.ascontiguousarray(arr, dtype=np.int64)
    bad = np.flatnonzero((arr < nb) | (arr > n - 1 - na))
    if bad.size:
        raise ValueError("cols[%d] = %d: its window of %d columns before and %d after leaves the result's %d columns"
                         % (bad[0], arr[bad[0]], nb, na, n))
    res = TriggeredResult(None, c, rows, nb, na, _pitch(n_lags), arr.size)
    return _run_into(
        res, "triggered", "%d channels, %d rows, %d lags" % (c, rows[1], n_lags), "fewer rows or a shorter window",
        lambda ptr: check(lib.gcwt_triggered(result.buffer.ptr, result.pitch, c, s, n, rows[0], rows[1],
                                             _ptr(arr, C.c_int64), arr.size, nb, na, ptr["amplitude"], ptr["power"],
                                             ptr["evoked"], ptr["vector"], ptr["itpc"], res.pitch)))


def band_rows(bands, frequencies):
    """The rows of bandpass() bands as a (B, 2) int32 array of (first, count): ``bands`` is one (f_lo, f_hi) pair or a
    sequence of them, in Hz, closed intervals, each resolved as coupling_rows does.  The ValueError that anything else
    raises names the band's index (``bands[k]``)."""
    try:
        one = not isinstance(bands, (str, bytes)) and len(bands) == 2 and all(np.ndim(v) == 0 and not isinstance(v, (str, bytes))
                                                                             for v in bands)
        seq = [bands] if one else list(bands)
    except TypeError:
        seq = None
    if not seq:
        raise ValueError("'bands' must be (f_lo, f_hi) in Hz or a non-empty sequence of such pairs, not %r" % (bands,))
    return np.array([coupling_rows(b, frequencies, "bands[%d]" % k) for k, b in enumerate(seq)], dtype=np.int32).reshape(-1, 2)


def _morlet_constants(w0):
    """(K1, K2) = (pi^-1/4 sqrt(2 pi) int psi dv / v, 2 sqrt(pi) int psi^2 dv / v) with psi(v) = exp(-(v - w0)^2 / 2) -
    exp(-w0^2 / 2 - v^2 / 2), by the midpoint rule on 2^19 cells of (0, w0 + 12] (psi / v stays finite at 0)."""
    n = 1 << 19
    v = (np.arange(n) + 0.5) * ((w0 + 12.0) / n)
    psi = np.exp(-0.5 * (v - w0) ** 2) - np.exp(-0.5 * w0 ** 2 - 0.5 * v ** 2)
    dv = (w0 + 12.0) / n
    return (np.pi ** -0.25 * np.sqrt(2 * np.pi) * np.sum(psi / v) * dv, 2 * np.sqrt(np.pi) * np.sum(psi ** 2 / v) * dv)


def band_weights(frequencies, wavelet):
    """The weights (g, h) of bandpass() for the rows at ``frequencies`` (Hz, strictly monotonic, at least 2) of a
    transform with ``wavelet`` (Morse or Morlet, its ``fs`` set for Morlet): float32 arrays of S entries, computed in
    float64 and cast once.  Host only.  d_r is the cell of row r in ln f -- half the distance between its two neighbours,
    the one-sided distance at either end of the grid: a property of the grid, not of a band.  The weights make a sinusoid
    of amplitude A, well inside a band that spans the wavelet's response, read envelope = A and power = A^2:
      Morse(gamma, beta), whose response peaks at 2, q = beta / gamma:  g_r = 2 d_r / C1,  h_r = 4 d_r / C2,
        C1 = 2 e^q q^-q Gamma(q) / gamma,  C2 = 4 e^2q (2q)^-2q Gamma(2q) / gamma;
      Morlet(w0), energy-normalised, sigma_r = (w0 + sqrt(2 + w0^2)) fs / (4 pi f_r) samples:
        g_r = 2 d_r / (sqrt(sigma_r) K1),  h_r = 4 d_r / (sigma_r K2)  (K1, K2: _morlet_constants)."""
    import math
    from .wave import morlet, morse
    f = np.asarray(frequencies, dtype=np.float64).ravel()
    if f.size < 2:
        raise ValueError("band_weights() needs at least 2 frequencies (a cell is the distance between neighbours), not %d" % f.size)
    if not np.all(np.isfinite(f)) or np.any(f <= 0):
        raise ValueError("the frequencies must be finite and positive")
    step = np.diff(np.log(f))
    if not (np.all(step > 0) or np.all(step < 0)):
        raise ValueError("the frequencies must be strictly monotonic")
    step = np.abs(step)
    d = np.concatenate((step[:1], 0.5 * (step[:-1] + step[1:]), step[-1:]))
    if isinstance(wavelet, morlet.Morlet):
        w0 = float(wavelet.w0)
        sigma = (w0 + np.sqrt(2 + w0 ** 2)) * float(wavelet.fs) / (4 * np.pi * f)
        k1, k2 = _morlet_constants(w0)
        g, h = 2 * d / (np.sqrt(sigma) * k1), 4 * d / (sigma * k2)
    elif isinstance(wavelet, morse.Morse):
        gamma, q = float(wavelet.gamma), float(wavelet.beta) / float(wavelet.gamma)
        c1 = 2 * math.exp(q - q * math.log(q) + math.lgamma(q)) / gamma
        c2 = 4 * math.exp(2 * q - 2 * q * math.log(2 * q) + math.lgamma(2 * q)) / gamma
        g, h = 2 * d / c1, 4 * d / c2
    else:
        raise ValueError("band_weights() knows Morse and Morlet wavelets, not %r" % (wavelet,))
    return g.astype(np.float32), h.astype(np.float32)


class _BandPlanes(_RowOpResult):
    """Planes of (C, B, N), one row for each of the B bands of ``rows`` and only those of ``outputs``, which a subclass's
    ``_OUTPUTS`` -- ((name, dtype), ...) in buffer order -- knows."""

    def __init__(self, buffer, n_channels, rows, n_cols, pitch, outputs):
        self.buffer, self.pitch, self.rows, self.outputs = buffer, int(pitch), rows, tuple(outputs)
        self.n_channels, self.n_bands, self.n_cols = int(n_channels), len(rows), int(n_cols)

    def _planes(self):
        lead = (self.n_channels, self.n_bands)
        return tuple((name, dtype, lead) for name, dtype in self._OUTPUTS if name in self.outputs), self.n_cols


class BandpassResult(_BandPlanes):
    """What bandpass() left on the device, each (C, B, N) with rows ``pitch`` elements apart in one DeviceBuffer and only
    those of ``outputs``: ``analytic`` complex64, ``envelope`` and ``power`` float32; ``rows``: (B, 2) of (first, count).
    ``to_host()`` brings them over; until ``free()`` a device-side consumer finds plane ``name`` at ``buffer.ptr +
    _offsets()[name]``."""
    _OUTPUTS = (("analytic", np.complex64), ("envelope", np.float32), ("power", np.float32))


def _outputs(outputs, table):
    """``outputs`` -- a name or a sequence of names of ``table`` = ((name, dtype), ...), at least one and each once -- as a
    tuple."""
    names = [name for name, _ in table]
    seq = (outputs,) if isinstance(outputs, str) else outputs
    try:
        ok = len(seq) >= 1 and all(isinstance(v, str) and v in names for v in seq) and len(set(seq)) == len(seq)
    except TypeError:
        ok = False
    if not ok:
        raise ValueError("'outputs' must name at least one of %s, each once, not %r" % (", ".join(names), outputs))
    return tuple(seq)


def _band_table(rows, n_scales):
    """``rows`` -- (B, 2) integers of (first, count), B >= 1, each a run of the result's ``n_scales`` rows -- as int32."""
    arr = np.asarray(rows)
    if arr.ndim != 2 or arr.shape[1] != 2 or arr.shape[0] < 1 or arr.dtype == np.bool_ or not np.issubdtype(arr.dtype, np.integer):
        raise ValueError("rows must be a (B, 2) integer array of (first, count) with B >= 1, not %s of shape %r" % (arr.dtype, arr.shape))
    return np.array([_row_range((int(a), int(b)), n_scales, "rows[%d]" % k) for k, (a, b) in enumerate(arr)], dtype=np.int32)


def _real_table(v, n, what, noun, owner, bound=None, quiet=True):
    """``v`` -- (n,) real numbers, one ``noun`` for each of ``owner`` -- as contiguous float32.  ``bound``: None, or what
    besides finite every entry must be: "" (nothing), "at least 0", "above 0".  ``quiet``: a number beyond float32's
    range becomes inf without numpy's overflow warning."""
    arr = np.asarray(v)
    if arr.shape != (n,) or arr.dtype == np.bool_ or not (np.issubdtype(arr.dtype, np.floating) or np.issubdtype(arr.dtype, np.integer)):
        raise ValueError("'%s' must hold one real %s for each of %s" % (what, noun, owner))
    with np.errstate(over="ignore" if quiet else None):
        arr = np.ascontiguousarray(arr, dtype=np.float32)
    if bound is not None and (not np.all(np.isfinite(arr)) or (bound == "at least 0" and np.any(arr < 0))
                              or (bound == "above 0" and np.any(arr <= 0))):
        raise ValueError("'%s' must be finite%s" % (what, " and " + bound if bound else ""))
    return arr


def _row_table(v, n_scales, what, noun, bound, quiet=True):
    """_real_table for one entry per row of the result."""
    return _real_table(v, n_scales, what, noun, "the result's %d rows" % n_scales, bound, quiet)


def _hz_per_cycle(v):
    """``v`` as the float32 the kernels take."""
    if not _is_number(v):
        raise ValueError("'hz_per_cycle' must be a finite number above 0 (fs / K), not %r" % (v,))
    with np.errstate(over="ignore"):
        hz = np.float32(v)
    if not np.isfinite(hz) or not hz > 0:
        raise ValueError("'hz_per_cycle' must be a finite number above 0 (fs / K), not %r" % (v,))
    return float(hz)


def bandpass(result, rows, g, h, outputs=("analytic", "envelope", "power")):
    """Band-limited analytic signals from the rows of a complex DeviceResult, computed where it lies (gcwt_bandpass;
    include/ghostcwt.h has the definition): for every band of ``rows`` -- (B, 2) of (first, count) as band_rows returns
    them; bands may overlap -- the sum of its rows weighted with ``g`` (analytic, envelope) and of their squared moduli
    weighted with ``h`` (power), (S,) weights as band_weights returns them; the one that no output needs may be None.
    Only the planes of ``outputs`` are allocated.  The result itself is only read.  -> BandpassResult, which stays on the
    device until ``to_host()`` / ``free()``."""
    c, s, n = _resident_complex(result, "bandpass", "a result sharded over several GPUs is not supported")
    outputs = _outputs(outputs, BandpassResult._OUTPUTS)
    arr = _band_table(rows, s)
    need_g, need_h = "analytic" in outputs or "envelope" in outputs, "power" in outputs
    g = _row_table(g, s, "g", "weight", "", quiet=False) if need_g else None
    h = _row_table(h, s, "h", "weight", "at least 0", quiet=False) if need_h else None
    res = BandpassResult(None, c, arr, n, _pitch(n), outputs)
    return _run_into(
        res, "bandpass", "%d channels, %d bands, %d columns, %s" % (c, len(arr), n, " + ".join(outputs)),
        "fewer bands or fewer outputs per call",
        lambda ptr: check(lib.gcwt_bandpass(result.buffer.ptr, result.pitch, c, s, n, _ptr(arr, C.c_int32), len(arr),
                                            _ptr(g, C.c_float), _ptr(h, C.c_float), ptr.get("analytic"),
                                            ptr.get("envelope"), ptr.get("power"), res.pitch)))


def ridge_weights(frequencies, wavelet):
    """The weights e of ridge() for the rows at ``frequencies`` (Hz) of a transform with ``wavelet`` (Morse or Morlet,
    its ``fs`` set for Morlet): float32, S entries, computed in float64 and cast once.  Host only.  e_r is the square of
    the amplitude gain that makes a sinusoid of amplitude A at f_r read sqrt(e_r |w_r|^2) = A on its own row:
      Morse, whose response peaks at 2 on every row: a row reads A as it is, e_r = 1;
      Morlet(w0), energy-normalised, sigma_r = (w0 + sqrt(2 + w0^2)) fs / (4 pi f_r) samples: the row reads
        sqrt(sigma_r) peak A,  peak = pi^-1/4 sqrt(pi / 2) psi(v_r),  v_r = (w0 + sqrt(2 + w0^2)) / 2 and psi as in
        _morlet_constants;  e_r = 1 / (sigma_r peak^2).  Without it the ridge of an energy-normalised transform leans
        to low frequencies."""
    from .wave import morlet, morse
    f = np.asarray(frequencies, dtype=np.float64).ravel()
    if f.size < 1:
        raise ValueError("ridge_weights() needs at least 1 frequency, not %d" % f.size)
    if not np.all(np.isfinite(f)) or np.any(f <= 0):
        raise ValueError("the frequencies must be finite and positive")
    if isinstance(wavelet, morlet.Morlet):
        w0 = float(wavelet.w0)
        v = (w0 + np.sqrt(2 + w0 ** 2)) / 2
        sigma = v * float(wavelet.fs) / (2 * np.pi * f)
        psi = np.exp(-0.5 * (v - w0) ** 2) - np.exp(-0.5 * w0 ** 2 - 0.5 * v ** 2)
        peak = np.pi ** -0.25 * np.sqrt(np.pi / 2) * psi
        e = 1.0 / (sigma * peak ** 2)
    elif isinstance(wavelet, morse.Morse):
        e = np.ones_like(f)
    else:
        raise ValueError("ridge_weights() knows Morse and Morlet wavelets, not %r" % (wavelet,))
    return e.astype(np.float32)


class RidgeResult(_BandPlanes):
    """What ridge() left on the device, each (C, B, N) with rows ``pitch`` elements apart in one DeviceBuffer and only
    those of ``outputs``: ``row`` int32, ``amplitude``, ``offset`` and ``frequency`` float32; ``rows``: (B, 2) of (first,
    count).  ``to_host()`` brings them over; until ``free()`` a device-side consumer finds plane ``name`` at ``buffer.ptr
    + _offsets()[name]``."""
    _OUTPUTS = (("row", np.int32), ("amplitude", np.float32), ("offset", np.float32), ("frequency", np.float32))


def _ridge_segments(segments, n_cols):
    seg = np.asarray(segments)
    if seg.ndim != 2 or seg.shape[1] != 2 or seg.shape[0] < 1 or seg.dtype == np.bool_ or not np.issubdtype(seg.dtype, np.integer):
        raise ValueError("'segments' must be an (n, 2) integer array of (start, stop) with n >= 1, not %s of shape %r"
                         % (seg.dtype, seg.shape))
    seg = np.ascontiguousarray(seg, dtype=np.int64)
    end = 0
    for k, (start, stop) in enumerate(seg):
        if stop <= start or start != end or stop > n_cols:
            raise ValueError("segments[%d] = [%d, %d): the segments must ascend, each hold a column and start where the one "
                             "before stops (here %d), from 0 to the result's %d columns" % (k, start, stop, end, n_cols))
        end = int(stop)
    if end != n_cols:
        raise ValueError("segments[%d] stops at %d: the segments must cover the result's %d columns" % (len(seg) - 1, end, n_cols))
    return seg


def ridge(result, rows, e, nu, hz_per_cycle, segments, outputs=("row", "amplitude", "frequency", "offset")):
    """The spectral ridge of bands of a complex DeviceResult and the instantaneous frequency on it, computed where the
    result lies (gcwt_ridge; include/ghostcwt.h has the definition): for every band of ``rows`` -- (B, 2) of (first,
    count) as band_rows returns them; bands may overlap -- and every column the ``row`` of largest e_r |w_r|^2 (-1 in a
    gap), its ``amplitude`` sqrt(e_r |w_r|^2), the parabolic sub-row ``offset`` and the ``frequency`` in Hz from the
    phase advance on that row between the neighbouring columns of the same segment.  ``e``: (S,) weights > 0 as
    ridge_weights returns them; ``nu``: (S,) >= 0, the phase advance each row expects per column, 2 pi f_r K / fs;
    ``hz_per_cycle``: fs / K; ``segments``: (n, 2) of (start, stop) as segments_of returns them, covering every column.
    Only the planes of ``outputs`` are allocated.  The result itself is only read.  -> RidgeResult, which stays on the
    device until ``to_host()`` / ``free()``."""
    c, s, n = _resident_complex(result, "ridge", "a result sharded over several GPUs is not supported")
    outputs = _outputs(outputs, RidgeResult._OUTPUTS)
    arr = _band_table(rows, s)
    e = _row_table(e, s, "e", "number", "above 0")
    nu = _row_table(nu, s, "nu", "number", "at least 0")
    hz = _hz_per_cycle(hz_per_cycle)
    seg = _ridge_segments(segments, n)
    res = RidgeResult(None, c, arr, n, _pitch(n), outputs)
    return _run_into(
        res, "ridge", "%d channels, %d bands, %d columns, %s" % (c, len(arr), n, " + ".join(outputs)),
        "fewer bands or fewer outputs per call",
        lambda ptr: check(lib.gcwt_ridge(result.buffer.ptr, result.pitch, c, s, n, _ptr(arr, C.c_int32), len(arr),
                                         _ptr(e, C.c_float), _ptr(nu, C.c_float), hz, _ptr(seg, C.c_int64), len(seg),
                                         ptr.get("row"), ptr.get("amplitude"), ptr.get("offset"), ptr.get("frequency"),
                                         res.pitch)))


def squeeze_edges(centres):
    """The cells of squeeze() around the centre frequencies ``centres`` (Hz, positive, strictly monotonic, at least 2 and at
    most 4096): -> (edges, descending).  ``edges``: float32, L + 1 entries, ascending: the geometric midpoints between
    neighbouring centres, the two ends extended by half their one-sided step in ln f; computed in float64 and cast once.
    ``descending``: the centres fall, so the cell of ``centres[k]`` is cell L - 1 - k of the ascending edges.  Host only.
    ValueError where the cast leaves two edges equal: it names the pair of centres that float32 cannot tell apart."""
    f = np.asarray(centres, dtype=np.float64).ravel()
    if f.size < 2:
        raise ValueError("squeeze_edges() needs at least 2 centre frequencies (a cell is the distance between neighbours), not %d" % f.size)
    if f.size > _lib.SQUEEZE_MAX_CELLS:
        raise ValueError("squeeze_edges() takes at most %d centre frequencies, not %d" % (_lib.SQUEEZE_MAX_CELLS, f.size))
    if not np.all(np.isfinite(f)) or np.any(f <= 0):
        raise ValueError("the centre frequencies must be finite and positive")
    step = np.diff(f)
    if not (np.all(step > 0) or np.all(step < 0)):
        raise ValueError("the centre frequencies must be strictly monotonic")
    descending = bool(f[0] > f[-1])
    ln = np.log(f[::-1] if descending else f)
    with np.errstate(over="ignore"):
        edges = np.exp(np.concatenate(([ln[0] - 0.5 * (ln[1] - ln[0])], 0.5 * (ln[:-1] + ln[1:]),
                                       [ln[-1] + 0.5 * (ln[-1] - ln[-2])]))).astype(np.float32)
    if not np.all(np.isfinite(edges)) or edges[0] <= 0:
        raise ValueError("the cells around the centre frequencies %g .. %g Hz leave float32's range" % (f.min(), f.max()))
    flat = np.flatnonzero(np.diff(edges) <= 0)
    if flat.size:
        # edges k and k + 1 enclose the ascending centre k: it lies too close to a neighbour
        k = min(int(flat[0]), f.size - 2)
        a, b = (f.size - 1 - k, f.size - 2 - k) if descending else (k, k + 1)
        raise ValueError("the centres %d and %d (%.17g and %.17g Hz) are too close: the edges of the cell between them are "
                         "the same float32" % (min(a, b), max(a, b), f[min(a, b)], f[max(a, b)]))
    return edges, descending


class SqueezeResult(_RowOpResult):
    """What squeeze() left on the device, rows ``pitch`` elements apart in one DeviceBuffer and only those of ``outputs``:
    ``coefficients`` complex64 and ``power`` float32, each (C, L, N) over the L cells; ``frequency`` float32 and ``index``
    int32, each (C, R, N) over the R input rows ``rows`` = (first, count).  ``to_host()`` brings them over; until
    ``free()`` a device-side consumer finds plane ``name`` at ``buffer.ptr + _offsets()[name]``."""

    def __init__(self, buffer, n_channels, rows, n_cells, n_cols, pitch, outputs):
        self.buffer, self.pitch, self.rows, self.outputs = buffer, int(pitch), tuple(rows), tuple(outputs)
        self.n_channels, self.n_rows, self.n_cells, self.n_cols = int(n_channels), int(rows[1]), int(n_cells), int(n_cols)

    _OUTPUTS = (("coefficients", np.complex64), ("power", np.float32), ("frequency", np.float32), ("index", np.int32))

    def _planes(self):
        lead = {"coefficients": (self.n_channels, self.n_cells), "power": (self.n_channels, self.n_cells),
                "frequency": (self.n_channels, self.n_rows), "index": (self.n_channels, self.n_rows)}
        return tuple((name, dtype, lead[name]) for name, dtype in self._OUTPUTS if name in self.outputs), self.n_cols


def _squeeze_cells(edges):
    arr = np.asarray(edges)
    if arr.ndim != 1 or arr.size < 2 or arr.dtype == np.bool_ or not (np.issubdtype(arr.dtype, np.floating) or np.issubdtype(arr.dtype, np.integer)):
        raise ValueError("'edges' must hold the L + 1 real edges of L >= 1 cells, not %s of shape %r" % (arr.dtype, arr.shape))
    if arr.size - 1 > _lib.SQUEEZE_MAX_CELLS:
        raise ValueError("'edges' holds %d cells, more than the %d that squeeze() takes" % (arr.size - 1, _lib.SQUEEZE_MAX_CELLS))
    with np.errstate(over="ignore"):
        arr = np.ascontiguousarray(arr, dtype=np.float32)
    if not np.all(np.isfinite(arr)) or np.any(arr <= 0):
        raise ValueError("'edges' must be finite and above 0")
    flat = np.flatnonzero(np.diff(arr) <= 0)
    if flat.size:
        raise ValueError("'edges' must be strictly ascending as float32: edges[%d] = %.9g is not above edges[%d] = %.9g"
                         % (flat[0] + 1, arr[flat[0] + 1], flat[0], arr[flat[0]]))
    return arr


def squeeze(result, rows, g, floor2, nu, hz_per_cycle, segments, edges, descending=False, outputs=("coefficients",)):
    """The synchrosqueezed transform of a run of rows of a complex DeviceResult, computed where the result lies
    (gcwt_squeeze; include/ghostcwt.h has the definition): every coefficient of the rows ``rows`` = (first, count) goes to
    the cell of ``edges`` -- (L + 1,) float32, > 0, strictly ascending, as squeeze_edges returns them -- that holds its own
    instantaneous ``frequency`` (ridge()'s, on every row), and what lands in a cell is added, weighted with ``g``, in
    ascending row order.  ``g``: (S,) finite weights as band_weights returns them; ``floor2``: (S,) >= 0, an entry whose
    |w|^2 is not above it stays out; ``nu``, ``hz_per_cycle``, ``segments``: exactly ridge()'s.  ``descending``: cell l is
    output row L - 1 - l.  ``index`` is the output row of every entry, -1 where it is out.  Only the planes of ``outputs``
    are allocated.  The result itself is only read.  -> SqueezeResult, which stays on the device until ``to_host()`` /
    ``free()``."""
    c, s, n = _resident_complex(result, "squeeze", "a result sharded over several GPUs is not supported")
    outputs = _outputs(outputs, SqueezeResult._OUTPUTS)
    first, count = _row_range(rows, s, "rows")
    g = _row_table(g, s, "g", "weight", "", quiet=False)
    floor2 = _row_table(floor2, s, "floor2", "number", "at least 0")
    nu = _row_table(nu, s, "nu", "number", "at least 0")
    hz = _hz_per_cycle(hz_per_cycle)
    seg = _ridge_segments(segments, n)
    edges = _squeeze_cells(edges)
    if not isinstance(descending, (bool, np.bool_)):
        raise ValueError("'descending' must be True or False, not %r" % (descending,))
    res = SqueezeResult(None, c, (first, count), edges.size - 1, n, _pitch(n), outputs)
    return _run_into(
        res, "squeeze", "%d channels, %d cells, %d rows, %d columns, %s" % (c, edges.size - 1, count, n, " + ".join(outputs)),
        "fewer cells, fewer outputs or an output_stride",
        lambda ptr: check(lib.gcwt_squeeze(result.buffer.ptr, result.pitch, c, s, n, first, count, _ptr(g, C.c_float),
                                           _ptr(floor2, C.c_float), _ptr(nu, C.c_float), hz, _ptr(seg, C.c_int64), len(seg),
                                           _ptr(edges, C.c_float), edges.size - 1, int(bool(descending)),
                                           ptr.get("coefficients"), ptr.get("power"), ptr.get("frequency"), ptr.get("index"),
                                           res.pitch)))


def _traces(buffer_ptr, pitch, n_traces, n_cols, what):
    """(pointer, pitch, n_traces, n_cols) of float32 traces on the device as the C entries take them."""
    ptr = buffer_ptr if isinstance(buffer_ptr, C.c_void_p) else C.c_void_p(buffer_ptr)
    if not ptr:
        raise ValueError("%s() needs traces on the device: the buffer has been freed" % what)
    for name, v in (("pitch", pitch), ("n_traces", n_traces), ("n_cols", n_cols)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s() takes '%s' as an integer, not %r" % (what, name, v))
    return ptr, int(pitch), int(n_traces), int(n_cols)


def trace_stats(buffer_ptr, pitch, n_traces, n_cols):
    """Per-trace statistics of float32 traces on the device -- ``n_traces`` rows of ``n_cols`` live columns, ``pitch``
    elements apart, at ``buffer_ptr`` (a c_void_p or an address) -- over the columns that are not exactly 0
    (gcwt_trace_stats; include/ghostcwt.h has the definition and the order of the float64 sums).  -> (n int64, mean
    float64, sd float64), each (n_traces,); mean and sd are 0 where n is.  Three numbers per trace cross to the host."""
    ptr, pitch, n_traces, n_cols = _traces(buffer_ptr, pitch, n_traces, n_cols, "trace_stats")
    n, mean, sd = np.zeros(max(n_traces, 0), np.int64), np.zeros(max(n_traces, 0)), np.zeros(max(n_traces, 0))
    check(lib.gcwt_trace_stats(ptr, pitch, n_traces, n_cols, _ptr(n, C.c_int64), _ptr(mean, C.c_double), _ptr(sd, C.c_double)))
    return n, mean, sd


_RUN_FIELDS = (("start", np.int64), ("stop", np.int64), ("peak_col", np.int64), ("peak", np.float32))


def trace_runs(buffer_ptr, pitch, n_traces, n_cols, lo):
    """The maximal runs of columns above ``lo`` -- (n_traces,) finite thresholds, one per trace -- of float32 traces on
    the device, with their peaks (gcwt_trace_runs; include/ghostcwt.h has the definition): found and compacted on the
    device, sized by a first call and written by a second into device arrays that are freed again.  -> dict of host
    arrays over the runs, ordered by trace and then by start: ``trace`` int64, ``start``, ``stop`` int64 (the run is
    the columns [start, stop)), ``peak_col`` int64 (the first column that holds the largest value), ``peak`` float32;
    and ``counts`` (n_traces,) int64: the runs of each trace.  28 bytes per run cross to the host."""
    ptr, pitch, n_traces, n_cols = _traces(buffer_ptr, pitch, n_traces, n_cols, "trace_runs")
    arr = _real_table(lo, n_traces, "lo", "threshold", "the %d traces" % n_traces, quiet=False)
    counts = np.zeros(n_traces, np.int64)

    def call(capacity, where):
        check(lib.gcwt_trace_runs(ptr, pitch, n_traces, n_cols, _ptr(arr, C.c_float), capacity, where["start"], where["stop"],
                                  where["peak_col"], where["peak"], _ptr(counts, C.c_int64)))

    call(0, dict.fromkeys((name for name, _ in _RUN_FIELDS)))
    total = int(counts.sum())
    out = {"trace": np.repeat(np.arange(n_traces, dtype=np.int64), counts)}
    if total == 0:
        out.update((name, np.zeros(0, dtype)) for name, dtype in _RUN_FIELDS)
    else:
        nbytes = sum(total * np.dtype(dtype).itemsize for _, dtype in _RUN_FIELDS)
        free, _ = device_memory()
        if nbytes > free:
            raise MemoryError("trace_runs() needs %d bytes on the device for %d runs and %d are free: a higher threshold"
                              % (nbytes, total, free))
        buf = DeviceBuffer(nbytes)
        try:
            offsets, end = {}, 0
            for name, dtype in _RUN_FIELDS:                 # (the int64 arrays first: each starts on 8 bytes)
                offsets[name] = end
                end += total * np.dtype(dtype).itemsize
            sized = counts.copy()
            call(total, {name: C.c_void_p(buf.ptr.value + off) for name, off in offsets.items()})
            if not np.array_equal(sized, counts):
                raise RuntimeError("trace_runs(): the traces changed between the two calls")
            out.update((name, buf.download((total,), dtype, offsets[name])) for name, dtype in _RUN_FIELDS)
        finally:
            buf.free()
    out["counts"] = counts
    return out


def trace_order(buffer_ptr, pitch, n_traces, n_cols, ranks, center=None):
    """Exact order statistics of float32 traces on the device (gcwt_trace_order; include/ghostcwt.h has the definition):
    per trace, over the columns that are not exactly 0, the value of every 0-based rank of ``ranks`` -- (n_traces, R) or
    (R,) for all traces, R = 1 .. 4 integers >= 0 -- in the total order of the bit patterns, a radix select on the
    device.  ``center``: None, or (n_traces,) finite values; the ranks are then those of ``|v - center|`` in float32.
    -> (n int64 (n_traces,): the columns that count; values float32 (n_traces, R): copies of the keys, bit for bit, and
    the NaN 0x7fc00000 where the rank is >= n).  8 + 4 R bytes per trace cross to the host."""
    ptr, pitch, n_traces, n_cols = _traces(buffer_ptr, pitch, n_traces, n_cols, "trace_order")
    arr = np.asarray(ranks)
    if arr.ndim == 1:
        arr = np.broadcast_to(arr, (max(n_traces, 0),) + arr.shape)
    if (arr.ndim != 2 or arr.shape[0] != n_traces or not 1 <= arr.shape[1] <= 4 or arr.dtype == np.bool_
            or not np.issubdtype(arr.dtype, np.integer)):
        raise ValueError("'ranks' must hold 1 .. 4 integer ranks, (R,) or one row for each of the %d traces, not %s of shape %r"
                         % (n_traces, arr.dtype, np.shape(ranks)))
    if arr.size and int(arr.min()) < 0:
        raise ValueError("'ranks' must be at least 0, not %d" % int(arr.min()))
    arr = np.ascontiguousarray(arr, dtype=np.int64)
    cen = None
    if center is not None:
        cen = _real_table(center, n_traces, "center", "value", "the %d traces" % n_traces)
        if not np.all(np.isfinite(cen)):
            raise ValueError("'center' must be finite in float32")
    n, values = np.zeros(arr.shape[0], np.int64), np.zeros(arr.shape, np.float32)
    check(lib.gcwt_trace_order(ptr, pitch, n_traces, n_cols, _ptr(cen, C.c_float), _ptr(arr, C.c_int64), arr.shape[1],
                               _ptr(n, C.c_int64), _ptr(values, C.c_float)))
    return n, values


MAD_TO_SD = 1.482602218505602                       # 1 / Phi^-1(3/4): the sd of a normal distribution from its MAD


def trace_median_mad(buffer_ptr, pitch, n_traces, n_cols):
    """Per-trace median and median absolute deviation of float32 traces on the device, over the columns that are not
    exactly 0, from exact order statistics (trace_order) and float64 on the host: with the values a, b of the ranks
    (n - 1) // 2 and n // 2, median = (a + b) / 2, which is exact; then, with center = float32(median) rounded once, the
    values c, d of the same ranks of |v - center| in float32, mad = (c + d) / 2.  -> (n int64, median float64, mad
    float64), each (n_traces,); both 0 where n is.  Three calls; a few numbers per trace cross to the host."""
    n, _ = trace_order(buffer_ptr, pitch, n_traces, n_cols, (0, 0))
    ranks = np.stack(((n - 1) // 2, n // 2), axis=1)
    ranks[n == 0] = 0
    _, mid = trace_order(buffer_ptr, pitch, n_traces, n_cols, ranks)
    with np.errstate(all="ignore"):
        median = np.where(n == 0, 0.0, (mid[:, 0].astype(np.float64) + mid[:, 1].astype(np.float64)) / 2)
        center = np.where(np.isfinite(median), median, 0.0).astype(np.float32)
    _, dev = trace_order(buffer_ptr, pitch, n_traces, n_cols, ranks, center)
    with np.errstate(all="ignore"):
        mad = np.where(n == 0, 0.0, (dev[:, 0].astype(np.float64) + dev[:, 1].astype(np.float64)) / 2)
    mad = np.where(np.isfinite(median), mad, np.nan)          # a median that is not finite has no deviations
    mad[n == 0] = 0.0
    return n, median, mad


def smooth_taps(sd_cols):
    """The centre and one side of a Gaussian window of standard deviation ``sd_cols`` columns, as trace_smooth takes
    them: half = int(4 sd_cols + 0.5) (scipy.ndimage.gaussian_filter1d's ``truncate=4``), w_k = exp(-k^2 / (2
    sd_cols^2)) for k = 0 .. half, normalised in float64 so that w_0 + 2 sum w_k = 1 and then rounded to float32 once.
    -> float32 (half + 1,).  ValueError where half is 0 (the window is narrower than a column) or above
    _lib.SMOOTH_MAX_HALF (the window counts in columns: an output stride shortens it)."""
    if not _is_number(sd_cols) or not np.isfinite(float(sd_cols)) or float(sd_cols) <= 0:
        raise ValueError("'sd_cols' must be a finite number of columns > 0, not %r" % (sd_cols,))
    sd = float(sd_cols)
    half = int(4 * sd + 0.5) if 4 * sd + 0.5 < 2.0 ** 62 else 2 ** 62
    if half < 1:
        raise ValueError("a Gaussian of sd %g columns is narrower than a column (4 sd < 0.5): nothing to smooth" % sd)
    if half > _lib.SMOOTH_MAX_HALF:
        raise ValueError("a Gaussian of sd %g columns reaches %d columns to either side, above the limit of %d: a larger "
                         "output_stride shortens it" % (sd, half, _lib.SMOOTH_MAX_HALF))
    k = np.arange(half + 1, dtype=np.float64)
    w = np.exp(-k * k / (2 * sd * sd))
    return (w / (w[0] + 2 * w[1:].sum())).astype(np.float32)


def segments_of(time, period, fs, n_cols):
    """The stretches of columns that belong together on the clock: a boundary lies before column j where ``|time[j] -
    time[j - 1] - period| > 0.5 / fs`` (trigger_columns' splice rule; ``period``: seconds per column, K / fs).  ``time``:
    the columns' times, or None: one segment.  -> (n, 2) int64 of (start, stop), ascending and covering [0, n_cols)."""
    n_cols = int(n_cols)
    if n_cols < 1:
        raise ValueError("segments_of() needs at least one column, not %d" % n_cols)
    if time is None:
        return np.array([[0, n_cols]], dtype=np.int64)
    t = np.asarray(time, dtype=np.float64).ravel()
    if t.size < n_cols:
        raise ValueError("'time' holds %d columns, fewer than the %d of the trace" % (t.size, n_cols))
    cut = np.flatnonzero(np.abs(np.diff(t[:n_cols]) - float(period)) > 0.5 / float(fs)) + 1
    edges = np.concatenate(([0], cut, [n_cols]))
    return np.ascontiguousarray(np.stack((edges[:-1], edges[1:]), axis=1), dtype=np.int64)


def trace_smooth(buffer_ptr, pitch, n_traces, n_cols, taps, segments=None, members=None):
    """A symmetric FIR along float32 traces on the device -- ``n_traces`` rows of ``n_cols`` live columns, ``pitch``
    elements apart, at ``buffer_ptr`` (a c_void_p or an address) -- computed there into a new buffer (gcwt_trace_smooth;
    include/ghostcwt.h has the definition, the order of the float32 operations and the bound of their rounding).
    ``taps``: w_0 .. w_half as smooth_taps returns them (``[1.0]``: no smoothing).  ``segments``: (n, 2) of (start,
    stop), ascending and disjoint, as segments_of returns them: a column's window ends where its segment does (zero
    extension) and a column in no segment is 0; None: one segment.  ``members``: trace indices whose mean, added in
    the order given, is the one trace that is smoothed; None: every trace on its own.  -> (DeviceBuffer, pitch of its
    rows, (rows, n_cols)): rows is 1 with ``members``, else n_traces.  The caller frees the buffer; the input is only
    read and nothing crosses to the host."""
    ptr, pitch, n_traces, n_cols = _traces(buffer_ptr, pitch, n_traces, n_cols, "trace_smooth")
    w = np.asarray(taps)
    if w.ndim != 1 or w.size < 1 or w.dtype == np.bool_ or not (np.issubdtype(w.dtype, np.floating) or np.issubdtype(w.dtype, np.integer)):
        raise ValueError("'taps' must be a 1-D array of real weights w_0 .. w_half, not %r" % (getattr(w, "shape", None),))
    with np.errstate(over="ignore"):
        w = np.ascontiguousarray(w, dtype=np.float32)
    seg = None
    if segments is not None:
        seg = np.asarray(segments)
        if seg.ndim != 2 or seg.shape[1] != 2 or seg.shape[0] < 1 or seg.dtype == np.bool_ or not np.issubdtype(seg.dtype, np.integer):
            raise ValueError("'segments' must be an (n, 2) integer array of (start, stop) with n >= 1, not %s of shape %r"
                             % (seg.dtype, seg.shape))
        seg = np.ascontiguousarray(seg, dtype=np.int64)
    mem = None
    if members is not None:
        mem = np.asarray(members)
        if mem.ndim != 1 or mem.size < 1 or mem.dtype == np.bool_ or not np.issubdtype(mem.dtype, np.integer):
            raise ValueError("'members' must be a 1-D array of at least one trace index, not %s of shape %r" % (mem.dtype, mem.shape))
        if mem.min() < 0 or mem.max() >= n_traces:
            raise ValueError("'members' must name traces 0 .. %d, not %d" % (n_traces - 1, mem.min() if mem.min() < 0 else mem.max()))
        mem = np.ascontiguousarray(mem, dtype=np.int32)
    n_out, out_pitch = (n_traces if mem is None else 1), _pitch(max(n_cols, 1))
    args = (ptr, pitch, n_traces, n_cols, _ptr(w, C.c_float), w.size - 1, _ptr(seg, C.c_int64), 0 if seg is None else len(seg),
            _ptr(mem, C.c_int32), 0 if mem is None else mem.size)
    if n_out < 1 or n_cols < 1:
        check(lib.gcwt_trace_smooth(*args, None, out_pitch))        # (refused in the library's words)
    nbytes = n_out * out_pitch * 4
    free, _ = device_memory()
    if nbytes > free:
        raise MemoryError("trace_smooth() needs %d bytes on the device for %d traces of %d columns and %d are free: fewer "
                          "traces per call" % (nbytes, n_out, n_cols, free))
    buf = DeviceBuffer(nbytes)
    try:
        check(lib.gcwt_trace_smooth(*args, buf.ptr, out_pitch))
    except Exception:
        buf.free()
        raise
    return buf, out_pitch, (n_out, n_cols)


def event_filter(trace, start, stop, peak_col, peak, hi, time_of_col, min_gap, min_duration, max_duration, period):
    """From the runs above the edge threshold (as trace_runs returns them: ordered by trace, then by start) to events.
    Pure NumPy on the compact list, in this order:
      1. keep the runs with ``peak > hi[trace]`` (``hi``: one threshold per trace);
      2. within a trace, merge neighbours whose gap time[start_next] - time[stop_prev - 1] is < ``min_gap`` seconds: the
         merged event spans both, its peak is the larger one, the earlier on a tie.  ``time_of_col``: the columns' times
         on the recording's clock, so that a gap between epochs counts with its real length (None: column j at j
         ``period``);
      3. drop the events whose duration (stop - start) ``period`` is below ``min_duration`` or above ``max_duration``
         (None: no upper limit); ``period``: seconds per column, K / fs.
    -> dict of ``trace``, ``start``, ``stop``, ``peak_col`` (int64) and ``peak`` (float32)."""
    trace, start, stop, peak_col = (np.asarray(v, dtype=np.int64).ravel() for v in (trace, start, stop, peak_col))
    peak = np.asarray(peak, dtype=np.float32).ravel()
    hi = np.atleast_1d(np.asarray(hi, dtype=np.float32))
    if not (trace.size == start.size == stop.size == peak_col.size == peak.size):
        raise ValueError("event_filter(): trace, start, stop, peak_col and peak must have one entry per run")
    min_gap, min_duration, period = _seconds(min_gap, "min_gap"), _seconds(min_duration, "min_duration"), float(period)
    max_duration = None if max_duration is None else _seconds(max_duration, "max_duration")
    keep = peak > hi[trace] if trace.size else np.zeros(0, bool)
    trace, start, stop, peak_col, peak = trace[keep], start[keep], stop[keep], peak_col[keep], peak[keep]
    if trace.size > 1 and min_gap > 0:
        if time_of_col is None:
            gap = (start[1:] - (stop[:-1] - 1)) * period
        else:
            t = np.asarray(time_of_col, dtype=np.float64).ravel()
            gap = t[start[1:]] - t[stop[:-1] - 1]
        joined = (trace[1:] == trace[:-1]) & (gap < min_gap)
        first = np.flatnonzero(np.concatenate(([True], ~joined)))            # the first run of every event
        last = np.concatenate((first[1:], [trace.size])) - 1
        top = np.maximum.reduceat(peak, first)
        group = np.cumsum(np.concatenate(([True], ~joined))) - 1
        at = np.minimum.reduceat(np.where(peak == top[group], np.arange(trace.size), trace.size), first)
        trace, start, stop, peak_col, peak = trace[first], start[first], stop[last], peak_col[at], top
    duration = (stop - start) * period
    keep = duration >= min_duration
    if max_duration is not None:
        keep &= duration <= max_duration
    return {"trace": trace[keep], "start": start[keep], "stop": stop[keep], "peak_col": peak_col[keep], "peak": peak[keep]}


def stride_columns(start, stop, stride):
    """Output columns of the samples [start, stop): the multiples of ``stride`` among them."""
    return max(0, -(-int(stop) // stride) - -(-int(start) // stride))


class CwtPlan:
    """One (n_channels, n_samples, frequencies, epochs) transform layout.

    Parameters mirror ``gcwt_params``; ``freqs_hz`` are the Morse peak
    frequencies in the order the output rows are wanted (``morlet_w0=w0``: the ``freq`` of
    ``Morlet(w0, freq, fs)`` instead, and ``gamma`` / ``beta`` are ignored).  ``output_stride`` K: row column j holds
    sample K j (gcwt_plan_set_output_stride), ceil(N / K) columns."""

    def __init__(self, n_samples, n_channels, fs, freqs_hz, *, gamma=3.0, beta=20.0,
                 epoch_bounds=None, output="amplitude", device=-1, band_eps=0.0, block=0,
                 max_fft_log2=0, normalization=None, order=0, precision=None, support_tol=0.0,
                 output_stride=1, morlet_w0=None):
        stride = output_stride_value(output_stride)
        self._handle = C.c_void_p()
        self.freqs = np.ascontiguousarray(freqs_hz, dtype=np.float64)
        if epoch_bounds is None:
            epoch_bounds = [[0, n_samples]]
        self.bounds = np.ascontiguousarray(epoch_bounds, dtype=np.int64).reshape(-1, 2)
        self.out_mode = _OUT_MODES[output] if isinstance(output, str) else int(output)
        p = _lib.Params()
        p.n_samples = int(n_samples)
        p.n_channels = int(n_channels)
        p.n_freqs = int(self.freqs.size)
        p.fs = float(fs)
        p.gamma = float(gamma)
        p.beta = float(beta)
        p.freqs_hz = self.freqs.ctypes.data_as(C.POINTER(C.c_double))
        p.n_epochs = int(self.bounds.shape[0])
        p.out_mode = self.out_mode
        p.epoch_bounds = self.bounds.ctypes.data_as(C.POINTER(C.c_int64))
        p.device = int(device)
        p.block = int(block)
        p.band_eps = float(band_eps)
        p.max_fft_log2 = int(max_fft_log2)
        # other members of the Morse family (morseutils.py:119-124, :181-196); transform()
        # itself always uses the first 'bandpass' wavelet (morse.py:84-91)
        if normalization not in (None, "bandpass", "energy"):
            raise ValueError("Normalization must be 'bandpass', or 'energy'")
        if not 0 <= int(order) <= 32:
            raise ValueError("order must be between 0 and 32")
        p.wavelet_flags = int(order) | (_lib.WAVELET_ENERGY if normalization == "energy" else 0)
        # morlet_w0: the Morlet wavelet of that non-dimensional frequency instead (GCWT_WAVELET_MORLET: gamma
        # carries w0, beta is ignored, no order or normalisation); freqs_hz are its ``freq``
        if morlet_w0 is not None:
            if normalization is not None or int(order) != 0:
                raise ValueError("a Morlet plan takes neither 'normalization' nor 'order'")
            if not float(morlet_w0) > 0:
                raise ValueError("Frequency ratio must be positive")
            p.gamma = float(morlet_w0)
            p.beta = 0.0
            p.wavelet_flags = _lib.WAVELET_MORLET
        # 'auto' (default): float64 forward transform and per-level low cut, the reference's dynamic range (it
        # computes in float64: transforms.py:142-143), with the scales at risk recomputed exactly; 'high': the same
        # without the recomputation; 'fast': float32 throughout; 'exact': no decimated path
        if precision not in (None, "default", "auto", "fast", "high", "exact"):
            raise ValueError("precision must be 'auto', 'fast', 'high' or 'exact'")
        p.precision = {None: 0, "default": 0, "auto": 4, "fast": 1, "high": 2, "exact": 3}[precision]
        p.support_tol = float(support_tol)
        check(lib.gcwt_plan_create(C.byref(self._handle), C.byref(p)))
        if stride != 1:
            check(lib.gcwt_plan_set_output_stride(self._handle, stride))
        self.n_samples, self.n_channels = int(n_samples), int(n_channels)
        self.n_freqs = int(self.freqs.size)
        self.output_stride = stride
        self.n_cols = stride_columns(0, self.n_samples, stride)     # output columns per row
        self.out_shape = (self.n_channels, self.n_freqs, self.n_cols)
        self.out_dtype = _OUT_DTYPE[self.out_mode]

    # -- description ------------------------------------------------------
    @property
    def info(self):
        i = _lib.PlanInfo()
        check(lib.gcwt_plan_get_info(self._handle, C.byref(i)))
        return {k: getattr(i, k) for k, _ in _lib.PlanInfo._fields_}

    def scale_info(self):
        s = self.n_freqs
        method = np.zeros(s, np.int32)
        dec = np.zeros(s, np.int32)
        halo = np.zeros(s, np.int32)
        hop = np.zeros(s, np.int32)
        length = np.zeros(s, np.int64)
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        check(lib.gcwt_plan_scale_info(self._handle, method.ctypes.data_as(i32p),
                                       dec.ctypes.data_as(i32p), halo.ctypes.data_as(i32p),
                                       hop.ctypes.data_as(i32p), length.ctypes.data_as(i64p)))
        theta_hi = np.zeros(s, np.float64)
        support = np.zeros(s, np.float64)
        n_bins = np.zeros(s, np.int32)
        f64p = C.POINTER(C.c_double)
        check(lib.gcwt_plan_scale_support(self._handle, theta_hi.ctypes.data_as(f64p),
                                          support.ctypes.data_as(f64p), n_bins.ctypes.data_as(i32p)))
        theta_neg = np.zeros(s, np.float64)
        check(lib.gcwt_debug_scale_theta_neg(self._handle, theta_neg.ctypes.data_as(f64p)))
        theta_lo = np.zeros(s, np.float64)
        check(lib.gcwt_debug_scale_theta_lo(self._handle, theta_lo.ctypes.data_as(f64p)))
        return {"method": method, "decimation": dec, "halo": halo, "hop": hop, "length": length,
                "theta_hi": theta_hi, "theta_neg": theta_neg, "theta_lo": theta_lo, "support": support,
                "n_bins": n_bins}

    # -- device -----------------------------------------------------------
    def upload(self):
        check(lib.gcwt_plan_upload(self._handle))

    def set_profiling(self, on=True):
        """True / 1: every stage between HIP events; 2: the synthesis kernels only (include/ghostcwt.h); False: none."""
        check(lib.gcwt_plan_set_profiling(self._handle, 2 if on == 2 and on is not True else (1 if on else 0)))

    def set_row_pitch(self, pitch_samples):
        """Row pitch (samples) of device output buffers; 0 = dense.  Use a multiple of 32
        when the row length is not one (see gcwt_plan_set_row_pitch)."""
        check(lib.gcwt_plan_set_row_pitch(self._handle, int(pitch_samples)))

    def precision_report(self):
        """After an execute with precision 'auto' (the default) or 'high': {"predicted": per scale, the loss to the
        float32 stages of its decimation level predicted from the recording's spectrum (relative to the scale's own
        output; 0 for scales on the exact paths), "worst", "rerouted": how many scales the last execute made again by
        the exact paths, "watched": False where the detector does not look -- plans whose segments take FFTs of 2^23 /
        2^24 points (kernels of millions of taps: DESIGN.md 8), every scale of which is then 'high''s}."""
        pred = np.zeros(self.n_freqs, np.float32)
        worst, n = C.c_float(0), C.c_int32(0)
        check(lib.gcwt_plan_precision_report(self._handle, pred.ctypes.data_as(C.POINTER(C.c_float)), C.byref(worst), C.byref(n)))
        if getattr(self, "_watched", None) is None:
            self._watched = all(p <= (1 << 22) for _, _, p in self.segments())
        return {"predicted": pred, "worst": float(worst.value), "rerouted": int(n.value), "watched": self._watched}

    def debug_precision_terms(self):
        """The two terms of the last execute's prediction (slot 0 of its last batch): float32 rounding of the level's
        stages, and what the level's slice of the spectrum leaves out; plus the energy each level's x_R held and the
        spectrum's band energies (sixteen bands per octave of the bin index) all of it is predicted from."""
        a, b = np.zeros(self.n_freqs, np.float32), np.zeros(self.n_freqs, np.float32)
        lv = np.zeros(max(1, self.info["n_levels"]), np.float32)
        bands = np.zeros(384, np.float32)
        f32p = C.POINTER(C.c_float)
        check(lib.gcwt_debug_precision_terms(self._handle, a.ctypes.data_as(f32p), b.ctypes.data_as(f32p), lv.ctypes.data_as(f32p),
                                             bands.ctypes.data_as(f32p)))
        return {"rounding": a, "left_out": b, "level_energy": lv, "band_energy": bands}

    def timings(self):
        t = _lib.Timings()
        check(lib.gcwt_get_timings(self._handle, C.byref(t)))
        return {k: getattr(t, k) for k, _ in _lib.Timings._fields_}

    def _host_result(self, shape, wide):
        """(array, flags) for a host result: float32/complex64, or the reference's
        float64/complex128 when ``wide`` (widened by the library while it copies)."""
        if not wide:
            return np.empty(shape, dtype=self.out_dtype), 0
        dt = np.complex128 if self.out_dtype == np.complex64 else np.float64
        return np.empty(shape, dtype=dt), _lib.OUT_F64

    def execute(self, x, wide=False):
        """x: array-like (C, N) -> ndarray out_shape (host in, host out)."""
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(self.n_channels, self.n_samples)
        out, flags = self._host_result(self.out_shape, wide)
        check(lib.gcwt_execute(self._handle, x.ctypes.data_as(C.c_void_p),
                               out.ctypes.data_as(C.c_void_p), flags))
        return out

    def execute_resident(self, x, result=None):
        """x: array-like (C, N) on the host; the result stays on the device: a DeviceResult (``result`` is reused
        when it is one of this shape).  Rows are padded to 32 samples (128-byte row starts: DESIGN.md 5)."""
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(self.n_channels, self.n_samples)
        self.upload()                           # (without a GPU this is where GCWT_ERR_NO_DEVICE is raised)
        pitch = (self.n_cols + 31) & ~31
        cplx = self.out_dtype == np.complex64
        if (result is None or result.buffer is None or result.shape != self.out_shape or result.pitch != pitch
                or result.is_complex != cplx):
            if result is not None:
                result.free()
            nbytes = self.n_channels * self.n_freqs * pitch * (8 if cplx else 4)
            result = DeviceResult(DeviceBuffer(nbytes), self.out_shape, pitch, cplx)
        self.set_row_pitch(pitch)
        try:
            check(lib.gcwt_execute(self._handle, x.ctypes.data_as(C.c_void_p), result.buffer.ptr, _lib.OUT_ON_DEVICE))
        finally:
            self.set_row_pitch(0)
        return result

    def execute_device(self, x_buf, out_buf):
        """Both buffers are DeviceBuffer (or raw c_void_p); returns when done."""
        xp = x_buf.ptr if isinstance(x_buf, DeviceBuffer) else x_buf
        op = out_buf.ptr if isinstance(out_buf, DeviceBuffer) else out_buf
        check(lib.gcwt_execute(self._handle, xp, op, _lib.X_ON_DEVICE | _lib.OUT_ON_DEVICE))

    def segments(self):
        """[(core_start, core_stop, fft_length)] of the time blocks the plan works in."""
        res = []
        for i in range(lib.gcwt_plan_segment_count(self._handle)):
            a, b, p = C.c_int64(), C.c_int64(), C.c_int64()
            check(lib.gcwt_plan_segment_info(self._handle, i, C.byref(a), C.byref(b), C.byref(p)))
            res.append((a.value, b.value, p.value))
        return res

    def execute_block(self, x, start, length, reuse_means=False, wide=False):
        """Samples [start, start+length) of every channel and scale from the whole
        recording x (C, N): ndarray (C, S, length) -- with an output stride, (C, S, columns): the samples of the
        range that the stride divides.  Host in, host out."""
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(self.n_channels, self.n_samples)
        cols = stride_columns(start, int(start) + int(length), self.output_stride)
        out, flags = self._host_result((self.n_channels, self.n_freqs, cols), wide)
        check(lib.gcwt_execute_block(self._handle, x.ctypes.data_as(C.c_void_p),
                                     out.ctypes.data_as(C.c_void_p), int(start), int(length),
                                     flags | (_lib.REUSE_MEANS if reuse_means else 0)))
        return out

    def execute_block_device(self, x_buf, out_buf, start, length, reuse_means=False):
        xp = x_buf.ptr if isinstance(x_buf, DeviceBuffer) else x_buf
        op = out_buf.ptr if isinstance(out_buf, DeviceBuffer) else out_buf
        flags = _lib.X_ON_DEVICE | _lib.OUT_ON_DEVICE | (_lib.REUSE_MEANS if reuse_means else 0)
        check(lib.gcwt_execute_block(self._handle, xp, op, int(start), int(length), flags))

    def filter_bank(self):
        b = self.info["block"]
        out = np.empty((self.n_freqs, b), dtype=np.complex64)
        check(lib.gcwt_filter_bank(self._handle, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def direct_kernel(self, scale):
        n = int(self.scale_info()["length"][scale])
        out = np.empty(n, dtype=np.complex64)
        check(lib.gcwt_direct_kernel(self._handle, int(scale),
                                     out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    # -- test hooks ---------------------------------------------------------
    def debug_levels(self, epoch=0):
        n = lib.gcwt_debug_level_count(self._handle)
        res = []
        for l in range(n):
            d, h, hp, nb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
            m = C.c_int64()
            check(lib.gcwt_debug_level_info(self._handle, epoch, l, C.byref(d), C.byref(h),
                                            C.byref(hp), C.byref(nb), C.byref(m)))
            sh = C.c_int32()
            check(lib.gcwt_debug_level_band_shift(self._handle, l, C.byref(sh)))
            cut = C.c_double()
            check(lib.gcwt_debug_level_low_cut(self._handle, l, C.byref(cut)))
            res.append({"decimation": d.value, "halo": h.value, "hop": hp.value,
                        "nblk": nb.value, "m": m.value, "band_shift": sh.value, "low_cut": cut.value})
        return res

    def debug_scale_lists(self):
        """Per level (the order of ``debug_levels``): {"rows": the scales in the order the synthesis kernels walk them,
        "n_plain": how many of them come before the half-sample ramp, "j_hi": first-layer inputs k_synth7 computes per
        entry (9 .. 16), zeros until the plan's tables are on the device (``upload`` / the first execute)}."""
        i32p = C.POINTER(C.c_int32)
        n_lv = lib.gcwt_debug_level_count(self._handle)
        first, plain = np.zeros(n_lv + 1, np.int32), np.zeros(max(1, n_lv), np.int32)
        n = lib.gcwt_debug_scale_lists(self._handle, first.ctypes.data_as(i32p), plain.ctypes.data_as(i32p), None, None, 0)
        if n < 0:
            check(n)
        rows, j_hi = np.zeros(max(1, n), np.int32), np.zeros(max(1, n), np.int32)
        rc = lib.gcwt_debug_scale_lists(self._handle, None, None, rows.ctypes.data_as(i32p), j_hi.ctypes.data_as(i32p), n)
        if rc < 0:
            check(rc)
        return [{"rows": rows[first[l]:first[l + 1]].copy(), "n_plain": int(plain[l]),
                 "j_hi": j_hi[first[l]:first[l + 1]].copy()} for l in range(n_lv)]

    def debug_work_items(self, kernel, batch=0):
        """The workgroup items of one synthesis kernel for launch batch ``batch`` (an index into ``debug_batches``),
        as the upload sends them (include/ghostcwt_debug.h: gcwt_debug_work_items; no device needed).  ``kernel``:
        "synth16", "synth7", "synth7_wide", "synth7_narrow", "interp" or "pipelined".  Returns {"items": a structured
        array, one record per item in launch order, "split": for "interp" / "pipelined" how many of them the first
        of the two launches takes, else None}."""
        fields = {"synth16": (0, ("level", "scale", "blk0", "nblk")),
                  "synth7": (1, ("level", "blk0", "rtile", "pad")),
                  "synth7_wide": (2, ("level", "blk0", "rtile", "pad")),
                  "synth7_narrow": (3, ("level", "blk0", "rtile", "pad")),
                  "interp": (4, ("level", "blk0", "pass0", "n_pass", "lo", "hi")),
                  "pipelined": (5, ("level", "blk0", "round0", "n_rounds"))}
        code, names = fields[kernel]
        n = lib.gcwt_debug_work_items(self._handle, code, int(batch), None, 0)
        if n < 0:
            check(n)
        flat = np.zeros(max(1, n), np.int32)
        rc = lib.gcwt_debug_work_items(self._handle, code, int(batch), flat.ctypes.data_as(C.POINTER(C.c_int32)), n)
        if rc < 0:
            check(rc)
        head = 1 if code >= 4 else 0
        items = np.ascontiguousarray(flat[head:n]).view(np.dtype([(f, np.int32) for f in names]))
        return {"items": items, "split": int(flat[0]) if head else None}

    def debug_mean_folded(self):
        """True when the last run summed the channels inside the forward column pass (include/ghostcwt_debug.h)."""
        return bool(lib.gcwt_debug_mean_folded(self._handle))

    def debug_graph_state(self):
        """1: executes replay a HIP graph, 0: not (yet), -1: capture failed, eager from then on."""
        return int(lib.gcwt_debug_graph_state(self._handle))

    def debug_blockconv(self):
        """Groups of the block-convolution scales: [{"scales": rows in order of kernel length, "hop", "back"}]."""
        i32p = C.POINTER(C.c_int32)
        n_bc = max(1, self.info["n_blockconv"])       # at most one group per scale
        arr = [np.zeros(n_bc, np.int32) for _ in range(4)]
        order = np.zeros(n_bc, np.int32)
        n = lib.gcwt_debug_blockconv_groups(self._handle, *[a.ctypes.data_as(i32p) for a in arr],
                                            order.ctypes.data_as(i32p), n_bc, n_bc)
        if n < 0:
            check(n)
        return [{"scales": order[arr[0][g]:arr[0][g] + arr[1][g]].tolist(), "hop": int(arr[2][g]), "back": int(arr[3][g])}
                for g in range(min(n, n_bc))]

    def debug_interp(self):
        """Per level: None when it is made by the FFT-per-sample kernels, else the interpolating
        synthesis' design -- q, factor I = R / q, alpha, err_bound, coef[2][I][8] -- and, under
        "demod", the demodulation bin of every scale of the plan (csrc/synthi.hip)."""
        n = lib.gcwt_debug_level_count(self._handle)
        f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        levels = []
        for l in range(n):
            q, fac, al, eb = C.c_int32(), C.c_int32(), C.c_double(), C.c_double()
            check(lib.gcwt_debug_interp_level(self._handle, l, C.byref(q), C.byref(fac), C.byref(al),
                                              C.byref(eb), None, 0))
            if q.value == 0:
                levels.append(None)
                continue
            coef = np.empty((2, fac.value, 8), dtype=np.float32)
            check(lib.gcwt_debug_interp_level(self._handle, l, None, None, None, None,
                                              coef.ctypes.data_as(f32p), coef.size))
            levels.append({"q": q.value, "factor": fac.value, "alpha": al.value,
                           "err_bound": eb.value, "coef": coef})
        demod = np.zeros(self.n_freqs, dtype=np.int32)
        check(lib.gcwt_debug_scale_demod(self._handle, demod.ctypes.data_as(i32p)))
        return {"levels": levels, "demod": demod}

    def debug_batches(self):
        """[(first_segment, count)] of the launch batches the plan's segments form."""
        res, seg, n = [], 0, lib.gcwt_plan_segment_count(self._handle)
        while seg < n:
            first, count = C.c_int32(), C.c_int32()
            check(lib.gcwt_debug_batch_of(self._handle, seg, C.byref(first), C.byref(count)))
            res.append((first.value, count.value))
            seg = first.value + max(1, count.value)
        return res

    def debug_exact_gain(self, scale, a, b):
        """G of one scale's reference kernel at theta = 2 pi a / b (host evaluation)."""
        a = np.ascontiguousarray(a, dtype=np.int64)
        out = np.empty(a.size, dtype=np.float64)
        check(lib.gcwt_debug_exact_gain(self._handle, int(scale), a.ctypes.data_as(C.POINTER(C.c_int64)),
                                        int(b), a.size, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def debug_fetch(self, what, channel=0, epoch=0, level=0):
        lv = self.debug_levels(epoch)
        if what == 0:
            # the STORED spectrum of the segment: its FFT length, or 2^22 bins of it in long mode (planner.h: p_store)
            p = self.segments()[epoch][2]
            n = p // max(1, p >> 22)
        elif what == 1:
            n = lv[level]["m"]
        else:
            n = lv[level]["nblk"] * self.info["block"]
        out = np.empty(n, dtype=np.complex64)
        check(lib.gcwt_debug_fetch(self._handle, what, channel, epoch, level,
                                   out.ctypes.data_as(C.POINTER(C.c_float)), n))
        return out

    def close(self):
        if self._handle:
            lib.gcwt_plan_destroy(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
