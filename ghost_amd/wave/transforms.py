"""Continuous wavelet transform with the reference's class surface
(ghost/wave/transforms.py:34-527), computed by libghostcwt on an MI355X.

``transform`` validates its arguments and builds the frequency grid exactly as
the reference does (transforms.py:109-182), then hands the whole per-scale /
per-epoch loop (transforms.py:187-224) to one ``gcwt_execute`` call.

Extensions (all default to reference behaviour):
  multichannel=True   accept (C, N) arrays / multi-signal ASAs; amplitude is (C, S, N)
  output='amplitude' | 'power' | 'complex'   what the device writes
  dtype=np.float64    dtype handed back (device arithmetic is float32)
  device=-1           HIP device ordinal (-1: current)
Deviations from reference quirks are listed in DESIGN.md.
"""
import logging
import time

import numpy as np

from . import wavelet as wavedef
from . import morse
from . import morlet
from ..formats import preprocessing as pre

__all__ = ["ContinuousWaveletTransform"]


class WaveletTransform:

    def __repr__(self):
        return self.__class__.__name__


class _Coherence:
    """What ContinuousWaveletTransform.coherence returns (host arrays)."""

    def __init__(self, coherence, cross, power, pairs, frequencies, time, window):
        self.coherence, self.cross, self.power, self.pairs = coherence, cross, power, pairs
        self.frequencies, self.time, self.window = frequencies, time, window


class _Coupling:
    """What ContinuousWaveletTransform.coupling returns (host arrays)."""

    def __init__(self, mvl, vector, amplitude, phase_frequencies, amplitude_frequencies, time, window, stats=None):
        self.mvl, self.vector, self.amplitude = mvl, vector, amplitude
        self.phase_frequencies, self.amplitude_frequencies = phase_frequencies, amplitude_frequencies
        self.time, self.window = time, window
        # surrogates=K only; None otherwise
        self.surrogate_mean, self.surrogate_sd, self.z, self.p, self.shifts, self.surrogates = (
            (stats or {}).get(k) for k in ("mean", "sd", "z", "p", "shifts", "surrogates"))


class _Triggered:
    """What ContinuousWaveletTransform.triggered returns (host arrays)."""

    def __init__(self, amplitude, power, evoked, vector, itpc, lags, frequencies, events_used, n_events):
        self.amplitude, self.power, self.evoked, self.vector, self.itpc = amplitude, power, evoked, vector, itpc
        self.lags, self.frequencies, self.events_used, self.n_events = lags, frequencies, events_used, n_events


class _Bandpass:
    """What ContinuousWaveletTransform.bandpass returns (host arrays)."""

    def __init__(self, analytic, envelope, power, bands, rows, frequencies, time):
        self.analytic, self.envelope, self.power = analytic, envelope, power
        self.bands, self.rows, self.frequencies, self.time = bands, rows, frequencies, time


class _Ridge:
    """What ContinuousWaveletTransform.ridge returns (host arrays)."""

    def __init__(self, row, amplitude, frequency, offset, bands, rows, frequencies, time, grid):
        self.row, self.amplitude, self.frequency, self.offset = row, amplitude, frequency, offset
        self.bands, self.rows, self.frequencies, self.time = bands, rows, frequencies, time
        self._grid = grid                                    # the transform's frequencies, all rows

    def grid_frequency(self):
        """The frequency of the grid at the sub-row position ``row + offset``, ln f interpolated linearly between the
        rows: float64, shaped like ``row``, NaN where ``row`` is -1.  NumPy on the host; needs the outputs 'row' and
        'offset'."""
        if self.row is None or self.offset is None:
            raise ValueError("grid_frequency() needs the outputs 'row' and 'offset'")
        at = self.row.astype(np.float64) + self.offset.astype(np.float64)
        out = np.exp(np.interp(at, np.arange(self._grid.size, dtype=np.float64), np.log(self._grid)))
        out[self.row < 0] = np.nan
        return out


class _Squeeze:
    """What ContinuousWaveletTransform.squeeze returns (host arrays)."""

    def __init__(self, coefficients, power, frequency, index, bin_frequencies, edges, rows, frequencies, time, min_amplitude):
        self.coefficients, self.power, self.frequency, self.index = coefficients, power, frequency, index
        self.bin_frequencies, self.edges, self.rows, self.frequencies = bin_frequencies, edges, rows, frequencies
        self.time, self.min_amplitude = time, min_amplitude


class _Events:
    """What ContinuousWaveletTransform.detect returns (host arrays)."""

    def __init__(self, events, per_channel, band, rows, frequencies, on, smooth=None, half=0, combined=False):
        # smooth: the Gaussian's sd in seconds or None; half: its reach in columns; combined: one trace for all channels
        self.smooth, self.half, self.combined = smooth, half, combined
        self.channel, self.start, self.stop, self.peak_time, self.peak = (events[k] for k in ("channel", "start", "stop", "peak_time", "peak"))
        self.start_col, self.stop_col, self.peak_col = events["start_col"], events["stop_col"], events["peak_col"]
        self.mean, self.sd, self.lo, self.hi = (per_channel[k] for k in ("mean", "sd", "lo", "hi"))
        self.n_columns, self.n_candidates = per_channel["n_columns"], per_channel["n_candidates"]
        # stats='median' / baseline=(t0, t1) only; None otherwise
        self.median, self.mad, self.baseline_cols = (per_channel.get(k) for k in ("median", "mad", "baseline_cols"))
        self.band, self.rows, self.frequencies, self.on = band, rows, frequencies, on

    def __len__(self):
        return len(self.channel)


def _fetched(res, squeeze=False):
    """The planes an engine operator left on the device, as host arrays -- without the channel axis where ``squeeze`` --;
    the device's copy is freed."""
    try:
        out = res.to_host()
    finally:
        res.free()
    return {k: v[0] for k, v in out.items()} if squeeze else out


def _baseline_columns(baseline, time, n_cols, period):
    """detect()'s ``baseline=(t0, t1)`` -> the columns [c0, c1) with t0 <= time < t1; ``time``: the columns' times or
    None (column j at j ``period``).  ValueError for anything but one non-empty stretch."""
    from .. import engine
    try:
        t0, t1 = baseline
        ok = all(engine._is_number(v) for v in (t0, t1))
    except (TypeError, ValueError):
        ok = False
    if not ok or not (np.isfinite(float(t0)) and np.isfinite(float(t1))):
        raise ValueError("detect(): 'baseline' must be None or (t0, t1), two finite numbers in seconds, not %r" % (baseline,))
    t0, t1 = float(t0), float(t1)
    if not t0 < t1:
        raise ValueError("detect(): 'baseline' is empty or reversed: t0 = %g is not below t1 = %g" % (t0, t1))
    t = np.arange(n_cols) * period if time is None else np.asarray(time, dtype=np.float64)[:n_cols]
    inside = np.flatnonzero((t >= t0) & (t < t1))
    if inside.size == 0:
        raise ValueError("detect(): 'baseline' (%g, %g) selects no column of the trace" % (t0, t1))
    c0, c1 = int(inside[0]), int(inside[-1]) + 1
    if c1 - c0 != inside.size:
        raise ValueError("detect(): 'baseline' (%g, %g) selects columns that are not one stretch: the times do not ascend" % (t0, t1))
    return c0, c1


class ContinuousWaveletTransform(WaveletTransform):
    """Continuous wavelet transform.

    Parameters
    ----------
    wavelet : ghost_amd.Wavelet, optional
        Default is ``Morse()`` (gamma=3, beta=20).  ``Morse(gamma, beta)`` or ``Morlet(w0)``: with a
        Morlet wavelet row ``f`` is the convolution with ``Morlet(w0, f, fs).get_wavelet()``, the
        frequency grid comes from ``Morlet.compute_freq_bounds`` and every keyword of ``transform()``
        works as with a Morse one (``w0 < 5`` is not admissible but is computed as asked).
    """

    def __init__(self, *, wavelet=None):
        if wavelet is None:
            wavelet = morse.Morse()
        self._wavelet = wavelet
        self._frequencies = None
        self._fs = None
        self._amplitude = None
        self._power = None
        self._coefficients = None
        self._time = None
        self._time_stride = 1               # output_stride of the last transform: time is timestamps[::K]
        self._stride = 1                    # ... kept after ``time`` has been asked for (triggered(): seconds per column)
        self._plan = None
        self._plan_key = None
        self.last_timings = None
        self._device_result = None          # the last transform's rows, still on the device
        self._pending = None                # (output, dtype, squeeze): what first access to a result attribute brings over
        self._last_kind = None              # ... of the result that has been brought over (fetch() after that)

    def transform(self, *args, multichannel=None, **kwargs):
        """Does a continuous wavelet transform; returns None and stores
        ``amplitude`` (and friends) on the object, like the reference.

        Parameters are those of ghost/wave/transforms.py:59-107: ``timestamps``,
        ``fs``, ``freq_limits``, ``freqs``, ``voices_per_octave``, ``parallel``
        (validated, then ignored: the GPU does all scales at once), ``verbose``.
        Beyond the reference: ``multichannel``, ``devices`` (with ``multichannel=True``: the GPUs the channels are
        sharded over, contiguous blocks, one plan and one host thread each -- ghost_amd/multi.py; the results stay on
        their devices and ``amplitude`` / ``fetch()`` stitch them), ``output`` ('amplitude', 'power', 'complex'), ``dtype``,
        ``lazy`` (default True: the result stays on the device when transform() returns and crosses PCIe on first
        access to ``amplitude`` / ``power`` / ``coefficients`` -- or piecewise through ``fetch()`` --; the device copy
        (C x S x N x 4 bytes, 8 for complex) is kept, for ``fetch()`` and for the next call to reuse, until the next
        transform() of another shape, ``release_device()`` or the object's end: many live objects hold many such
        buffers; False: the result is on the host when transform() returns, as in the reference),
        ``device`` and ``precision`` ('auto', the default: the forward FFT in float64 like the reference's
        arithmetic, transforms.py:142-143, and the scales a mains line or the like inside their decimation band
        would cost more than 1.5e-6 of their peak are recomputed by exact FFT convolution, logged; 'high': the same
        without the recomputation, it only warns; 'fast': float32 throughout; 'exact': every scale by FFT
        convolution with its literal kernel, 3 - 9 x slower), ``output_stride`` (an integer K >= 1, default 1: only
        every K-th sample of the recording's own grid is computed and kept -- column j holds sample K j, ceil(N / K)
        columns, exactly the full-rate result's ``[..., ::K]``, gaps between epochs 0 as always; ``time`` is
        ``timestamps[::K]`` and ``amplitude`` / ``power`` / ``coefficients`` / ``fetch()`` count columns.  Point
        sampling: no average over the K samples).
        """
        if multichannel is None:
            multichannel = False
        if multichannel not in (True, False):
            raise ValueError("'multichannel' must be either True or False")
        if multichannel:
            return self._transform_any(*args, **kwargs)
        return self._transform_one(*args, **kwargs)

    def _transform_one(self, data, **kwargs):
        return self._run(data, squeeze=True, **kwargs)

    def _transform_any(self, data, **kwargs):
        return self._run(data, squeeze=False, **kwargs)

    _transform_one._public_name = _transform_any._public_name = "transform"
    # the reference decorates transform() itself (transforms.py:57-58)
    _transform_one = pre.standardize_asa(x="data", fs="fs", n_signals=1, class_method=True,
                                         abscissa_vals="timestamps", defer_abscissa=True)(_transform_one)
    _transform_any = pre.standardize_asa(x="data", fs="fs", n_signals=None, class_method=True,
                                         abscissa_vals="timestamps", defer_abscissa=True)(_transform_any)

    def _run(self, data, *, squeeze, timestamps=None, fs=None, freq_limits=None, freqs=None,
             voices_per_octave=None, parallel=None, verbose=None, output=None, dtype=None,
             device=None, devices=None, precision=None, lazy=None, output_stride=None, **kwargs):
        from ..engine import output_stride_value
        stride = output_stride_value(1 if output_stride is None else output_stride)   # before anything else
        self.fs = fs                        # validates (transforms.py:109)
        self._time = timestamps
        self._time_stride = stride
        self._stride = stride

        if freqs is not None and freq_limits is not None:
            raise ValueError("freq_limits and freqs cannot both be used at the"
                             " same time. Either specify one or the either, or"
                             " leave both as unspecified")
        if voices_per_octave is None:
            voices_per_octave = 10
        if voices_per_octave not in np.arange(4, 50, step=2):
            raise ValueError("'voices_per_octave' must be an even number"
                             " between 4 and 48, inclusive")
        if parallel is None:
            parallel = False
        if parallel not in (True, False):
            raise ValueError("'parallel' must be either True or False")
        if verbose is None:
            verbose = False
        if verbose not in (True, False):
            raise ValueError("'verbose' must be either True or False")
        if output is None:
            output = "amplitude"
        if output not in ("amplitude", "power", "complex"):
            raise ValueError("'output' must be 'amplitude', 'power' or 'complex'")
        if dtype is None:
            dtype = np.float64
        if devices is not None:
            # several GPUs of one node: contiguous channel blocks, one plan and one host thread per entry
            # (ghost_amd/multi.py); an entry may repeat (two slots on one device)
            if device is not None:
                raise ValueError("'device' and 'devices' cannot both be used")
            devices = [int(d) for d in np.atleast_1d(devices)]
            if not devices or min(devices) < 0:
                raise ValueError("'devices' must be a non-empty list of device indices")
            if len(devices) == 1:
                device, devices = devices[0], None
        if device is None:
            device = -1
        if lazy is None:
            lazy = True
        if lazy not in (True, False):
            raise ValueError("'lazy' must be either True or False")

        epoch_bounds = kwargs.pop("epoch_bounds", None)
        # (N, C) column signals from the adapter -> (C, N) rows for the device
        arr = np.asarray(data).reshape(data.shape[0], -1).T
        if arr.dtype != np.float32:
            # The reference works on a float64 copy with the global mean removed (transforms.py:142-143).  The
            # device takes float32: wider input loses its mean here, in its own precision, so that an offset
            # far above the signal (raw counts, a DC level of 1e7 x the fluctuation) does not cost the cast
            # the signal's bits; the device removes what is left of the mean in float64 as it always does.
            arr = arr.astype(np.float64, copy=False)
            arr = arr - arr.mean(axis=1, keepdims=True)
        x = np.ascontiguousarray(arr, dtype=np.float32)
        n_channels, n_samples = x.shape
        if epoch_bounds is None:
            epoch_bounds = np.array([[0, n_samples]])
        epoch_bounds = np.asarray(epoch_bounds).astype(np.int64).reshape(-1, 2)
        lengths = np.diff(epoch_bounds, axis=1).astype(int)

        freq_bounds_ref = self._norm_radians_to_hz(           # transforms.py:147-149
            self.wavelet.compute_freq_bounds(np.min(lengths)))

        if freqs is not None:
            freqs = np.sort(np.asarray(freqs, dtype=np.float64))
            # reference uses freqs[1] as the upper bound (transforms.py:155), which masks
            # nearly every request; the evident intent is the largest frequency
            lb, ub = self._check_freq_bounds([freqs[0], freqs[-1]], freq_bounds_ref)
            f = freqs[np.logical_and(freqs >= lb, freqs <= ub)]
        else:
            if freq_limits is not None:
                freq_limits = np.sort(freq_limits)
                f_low, f_high = self._check_freq_bounds([freq_limits[0], freq_limits[1]],
                                                        freq_bounds_ref)
            else:
                f_low, f_high = freq_bounds_ref
            n_octaves = np.log2(f_high / f_low)                # transforms.py:169-173
            j = np.arange(np.floor(n_octaves * voices_per_octave) + 1)
            f = f_high / 2 ** (j / voices_per_octave)
        self._frequencies = f
        self._wavelet.fs = self._fs                            # transforms.py:179

        from ..engine import CwtPlan   # needs the built library; no CPU fallback
        from .. import _lib
        if precision not in (None, "auto", "high", "fast", "exact"):
            raise ValueError("'precision' must be 'auto' (default: 'high', with the scales a strong in-band "
                             "interferer would cost their low bits made again by the exact paths), 'high' (the "
                             "reference's float64 dynamic range in front of the float32 synthesis), 'fast' (float32 "
                             "throughout) or 'exact' (no decimated path: every scale's float32 stages see only what "
                             "its own filter lets through)")
        # the wavelet family and its parameters, as the plan key and as CwtPlan's keywords
        if isinstance(self._wavelet, morlet.Morlet):
            family = {"morlet_w0": float(self._wavelet.w0)}
        else:
            family = {"gamma": float(self._wavelet.gamma), "beta": float(self._wavelet.beta)}
        key = (n_samples, n_channels, float(self._fs), f.tobytes(), tuple(sorted(family.items())),
               epoch_bounds.tobytes(), output, int(device), precision,
               None if devices is None else tuple(devices), stride)
        if self._plan is None or self._plan_key != key:
            if self._plan is not None:
                self._plan.close()
                self._plan = None
            if devices is not None and n_channels > 1:
                from ..multi import ShardedPlan
                self._plan = ShardedPlan(n_samples, n_channels, self._fs, f, devices, epoch_bounds=epoch_bounds,
                                         output=output, precision=precision, output_stride=stride, **family)
            else:
                self._plan = CwtPlan(n_samples, n_channels, self._fs, f, epoch_bounds=epoch_bounds,
                                     output=output, device=device if devices is None else devices[0],
                                     precision=precision, output_stride=stride, **family)
            self._plan_key = key
        self._plan.set_profiling(bool(verbose))
        start_time = time.time()
        # The rows stay on the device (engine.DeviceResult); what the reference keeps as whole host arrays
        # (transforms.py:203-204, 496-527) is brought over by the first access to the attribute: into page-locked
        # memory at the link's rate; float64 (the reference's dtype) crosses as float32 and is widened as it lands.
        self._amplitude = self._power = self._coefficients = None
        # (the device buffer of the previous call is reused: until this execute has succeeded nothing describes it)
        self._pending = None
        self._device_result = self._plan.execute_resident(x, self._device_result)
        self._pending = (output, np.dtype(dtype), squeeze)
        # the detector's verdict (precision 'auto' / 'high': DESIGN.md 3): scales whose decimation level holds far more
        # than they do -- a mains line inside an analysed band -- were made again by the exact paths ('auto'), or are
        # reported ('high')
        self.precision_report = None
        if precision in (None, "auto", "high"):
            rep = self.precision_report = self._plan.precision_report()
            if not rep["watched"] and precision != "high":
                # kernels of millions of taps: FFTs of 2^23 / 2^24 points, combined from interleaved transforms -- the
                # detector's band sums are not made there: said once per call, never silently
                logging.warning("precision='auto' does not watch transforms of more than 2^22 points (kernels of millions "
                                "of taps): every scale holds what precision='high' returns; precision='exact' for "
                                "recordings with interference far above the signal inside the analysed band")
            if rep["rerouted"] < 0:
                logging.warning("{} of {} scales are predicted to lose up to {:.1e} of their peak to the float32 stages and "
                                "could not all be recomputed exactly (no device memory for the exact paths: {}); they hold "
                                "what precision='high' returns".format(-rep["rerouted"], f.size, rep["worst"],
                                                                        _lib.lib.gcwt_last_error().decode("utf-8", "replace")))
            elif rep["rerouted"]:
                logging.warning("{} of {} scales were recomputed by exact FFT convolution: the recording holds up to {:.0f} x "
                                "more in their decimation bands than in the scales themselves (predicted float32 loss {:.1e} "
                                "of a scale's peak; precision='high' skips this, 'exact' does it for every scale)"
                                .format(rep["rerouted"], f.size, rep["worst"] / 1.6e-7, rep["worst"]))
            elif precision == "high" and rep["worst"] > 1.5e-6:
                logging.warning("precision='high': the float32 stages are predicted to cost some scales {:.1e} of their "
                                "peak (the recording holds far more inside their decimation bands than they do); "
                                "precision='auto' (the default) recomputes those scales exactly".format(rep["worst"]))
        if verbose:
            self.last_timings = self._plan.timings()
            print("Elapsed time (only wavelet convolution): {} seconds"
                  " to analyze {} frequencies".format(time.time() - start_time, f.size))
            print("device stages (ms): {}".format(self.last_timings))
        if not lazy:
            self._materialize()

    # -- results: on the device until asked for ------------------------------------
    def _materialize(self):
        if self._pending is None or self._device_result is None:
            return
        output, dtype, squeeze = self._pending
        self._last_kind = self._pending
        self._pending = None
        wide = dtype == np.dtype(np.float64)
        if output == "complex":
            res = self._device_result.to_host(np.complex128 if wide else np.complex64)
        else:
            res = self._device_result.to_host(np.float64 if wide else np.float32)
            res = res.astype(dtype, copy=False)
        if squeeze:
            res = res[0]
        if output == "amplitude":
            self._amplitude = res
        elif output == "power":
            self._power = res
        else:
            self._coefficients = res

    @property
    def device_result(self):
        """The last transform's rows on the device (engine.DeviceResult: ``buffer.ptr``, ``shape`` (C, S, N),
        ``pitch``), or None.  Valid until the next transform() or ``release_device()``."""
        return self._device_result

    def fetch(self, scales=None, start=0, stop=None, dtype=None):
        """Scales ``scales`` (a slice; None = all) and columns [start, stop) of the last transform (samples; with an
        output stride K, column j is sample K j), straight from
        the device, without bringing the rest of the result over: ndarray (S', n) -- (C, S', n) for multichannel
        transforms -- of what ``output=`` selected.  dtype: float32 or float64 (default: the transform's)."""
        if self._device_result is None:
            raise ValueError("no transform on the device (call transform() first)")
        out_kind, t_dtype, squeeze = self._pending if self._pending is not None else self._last_kind
        dtype = np.dtype(t_dtype if dtype is None else dtype)
        wide = dtype == np.dtype(np.float64)
        if out_kind == "complex":
            res = self._device_result.to_host(np.complex128 if wide else np.complex64, scales, start, stop)
        else:
            res = self._device_result.to_host(np.float64 if wide else np.float32, scales, start, stop)
        return res[0] if squeeze else res

    def _resident_rows(self, what, one_device="works", sharded="which is not supported"):
        """(the last transform's DeviceResult, squeeze) for operator ``what``; ValueError where there is none, it is not
        complex, or it is sharded over several devices."""
        from .. import engine
        if self._device_result is None or (self._pending is None and self._last_kind is None):
            raise ValueError("no transform on the device (call transform() first)")
        out_kind, _, squeeze = self._pending if self._pending is not None else self._last_kind
        if out_kind != "complex":
            raise ValueError("%s() needs the complex coefficients: the last transform was output='%s', "
                             "not output='complex'" % (what, out_kind))
        if not isinstance(self._device_result, engine.DeviceResult):
            raise ValueError("%s() %s on one device: the last transform was sharded over several "
                             "(devices=[...]), %s" % (what, one_device, sharded))
        return self._device_result, squeeze

    def _phase_clock(self, f, n_cols):
        """What ridge() and squeeze() turn a phase advance into a frequency with, for rows at ``f`` Hz and ``n_cols``
        columns: (the columns' times or None, nu = 2 pi f K / fs, hz_per_cycle = fs / K, the segments of the clock)."""
        from .. import engine
        stride, fs = self._stride, float(self._fs)
        t = self.time
        t = None if t is None else np.asarray(t)
        return t, 2 * np.pi * f * stride / fs, fs / stride, engine.segments_of(t, stride / fs, fs, n_cols)

    def coherence(self, pairs=None, *, seed=None, window):
        """Wavelet coherence and cross-spectra between channels of the last transform, reduced on the device over bins
        of ``window`` columns (an integer >= 2; with an output stride K a column is K samples) -- the transform must
        have been ``multichannel=True, output='complex'`` with at least 2 channels on one device.  ``pairs``: (P, 2)
        channel indices; ``seed=c``: channel c against every other; neither: all pairs a < b.  With Sxy the sum of
        W[a] conj(W[b]) over a bin of cnt columns, Sxx and Syy those of |W[a]|^2 and |W[b]|^2, the returned object has
        ``coherence`` (P, S, B) float32 = |Sxy|^2 / (Sxx Syy) in [0, 1], ``cross`` (P, S, B) complex64 = Sxy / cnt
        (angle > 0: channel b lags channel a), ``power`` (C, S, B) float32 = Sxx / cnt of every channel, ``pairs``
        (P, 2), ``frequencies`` (S,), ``time`` (B,): the time of each bin's first column, and ``window``.  Bins are
        plain column ranges, B = ceil(columns / window), the last one may be short; a bin inside a gap between epochs
        is exactly 0 in all three.  A bin shorter than the wavelet's duration at a scale reads close to 1 whatever
        the signals -- a property of the estimator (one effective sample), not an error: choose ``window`` as several
        periods of the lowest frequency of interest.  Only the reduced arrays cross to the host; the resident result,
        ``fetch()`` and the result attributes are untouched."""
        from .. import engine
        window = engine.bin_window(window)
        result, squeeze = self._resident_rows("coherence", "pairs channels", "and pairs across devices are not supported")
        if squeeze or result.shape[0] < 2:
            raise ValueError("coherence() relates channels: the last transform must be multichannel=True with at "
                             "least 2 channels")
        pairs = engine.coherence_pairs(pairs, seed, result.shape[0])
        out = _fetched(engine.coherence(result, pairs, window))
        t = self.time
        return _Coherence(out["coherence"], out["cross"], out["power"], pairs.astype(np.int64),
                          np.array(self._frequencies), None if t is None else np.asarray(t)[::window], window)

    def coupling(self, *, phase, amplitude, window, surrogates=None, min_shift=None, seed=0, keep_surrogates=False):
        """Phase-amplitude coupling inside each channel of the last transform -- does the amplitude of a fast band ride
        on the phase of a slow one? --, reduced on the device over bins of ``window`` columns (an integer >= 2; with
        an output stride K a column is K samples).  The transform must have been ``output='complex'`` on one device.
        ``phase`` and ``amplitude``: (f_lo, f_hi) in Hz; the rows whose frequency lies in the closed interval (P phase
        rows, A amplitude rows; the bands may overlap).  With u = W[p] / |W[p]| (0 where that is 0), M the sum of
        |W[a]| u over a bin of cnt columns and S that of |W[a]|, the returned object has ``vector`` (C, P, A, B)
        complex64 = M / cnt (its angle: the phase of row p at which row a is strongest), ``mvl`` (C, P, A, B) float32 =
        |M| / S in [0, 1], the normalised mean vector length (0: no preferred phase, 1: all amplitude at one phase),
        ``amplitude`` (C, A, B) float32 = S / cnt, ``phase_frequencies`` (P,), ``amplitude_frequencies`` (A,),
        ``time`` (B,): the time of each bin's first column, and ``window``; after the reference's single-channel call
        the channel axis is dropped.  Bins are plain column ranges, B = ceil(columns / window), the last one may be
        short; a bin inside a gap between epochs is exactly 0 in all three.  A bin shorter than about one period of
        the phase row reads high whatever the signal -- a property of the estimator (one effective sample), not an
        error: choose ``window`` as several periods of the lowest phase frequency.  A raw mvl is therefore read against
        its shift surrogates (Canolty et al. 2006): ``surrogates=K`` (an int in 2 .. 4096; ``window`` at most
        2048 columns then, GCWT_COUPLING_SURROGATES_MAX_WINDOW; C: gcwt_coupling_surrogates) draws K shifts with
        ``engine.surrogate_shifts(K, window, min_cols, seed)`` -- one list for every channel, cell and bin; ``min_shift`` in
        seconds, default one period of the lowest selected phase frequency, becomes ``min_cols = ceil(min_shift fs /
        stride)`` columns --, and for each shift L moves the amplitude row circularly inside each bin, |W[a]| at column b
        + (r + L mod cnt) mod cnt against u at b + r, and makes the mvl again on the device, in coupling()'s arithmetic
        and order.  The object then also has ``surrogate_mean`` and ``surrogate_sd`` (C, P, A, B) float32 (sums in
        float64, the sd with K - 1), ``z`` = (mvl - mean) / sd (float64 on the host, 0 where sd == 0, float32), ``p`` =
        (1 + the number of surrogates >= mvl) / (K + 1) float32, ``shifts`` (K,) int64 and, with ``keep_surrogates``,
        ``surrogates`` (K, C, P, A, B) float32, whose plane of a shift 0 has the bits of ``mvl``; without ``surrogates``
        these are None and the call is what it was.  The shift is bin-local and circular: it keeps the non-stationarity
        of the recording out of the null, never reads across a gap and leaves S fixed.  The price: the surrogates
        decorrelate only if a bin spans several coherence times of the phase rhythm -- a perfectly periodic rhythm gives z
        near 0 however strong its coupling --, a bin partly inside a gap has surrogates biased low, and a bin wholly
        inside a gap is 0 everywhere with p = 1 and z = 0.  Only the reduced arrays cross to the host; the resident
        result, ``fetch()`` and the result attributes are untouched."""
        from .. import engine
        window = engine.bin_window(window)
        result, squeeze = self._resident_rows("coupling")
        f = np.array(self._frequencies)
        phase_rows = engine.coupling_rows(phase, f, "phase")
        amp_rows = engine.coupling_rows(amplitude, f, "amplitude")
        f_phase = f[phase_rows[0]:phase_rows[0] + phase_rows[1]]
        shifts = None
        if surrogates is not None:
            if window > engine._lib.COUPLING_SURROGATES_MAX_WINDOW:
                raise ValueError("coupling(): with surrogates, window = %d columns is above the largest bin the device "
                                 "holds, %d columns (GCWT_COUPLING_SURROGATES_MAX_WINDOW): a shorter window or an "
                                 "output_stride" % (window, engine._lib.COUPLING_SURROGATES_MAX_WINDOW))
            per_col = float(self._stride) / float(self._fs)      # seconds per column
            if min_shift is None:
                min_cols = int(np.ceil(float(self._fs) / (self._stride * float(f_phase.min()))))
            else:
                if not engine._is_number(min_shift) or not np.isfinite(float(min_shift)) or float(min_shift) <= 0:
                    raise ValueError("coupling(): 'min_shift' must be a finite number of seconds > 0, not %r" % (min_shift,))
                min_cols = max(1, int(np.ceil(float(min_shift) / per_col)))
            shifts = engine.surrogate_shifts(surrogates, window, min_cols, seed)
        out = _fetched(engine.coupling(result, phase_rows, amp_rows, window))
        stats = None
        if shifts is not None:
            stats = _fetched(engine.coupling_surrogates(result, phase_rows, amp_rows, window, shifts, keep=keep_surrogates))
            mean, sd = stats["mean"].astype(np.float64), stats["sd"].astype(np.float64)
            stats["z"] = np.where(sd > 0, (out["mvl"].astype(np.float64) - mean) / np.where(sd > 0, sd, 1.0), 0.0).astype(np.float32)
            stats["p"] = ((1.0 + stats.pop("count_ge")) / (shifts.size + 1.0)).astype(np.float32)
            stats["shifts"] = shifts
        if squeeze:
            out = {k: v[0] for k, v in out.items()}
            if stats is not None:
                stats = {k: v if k == "shifts" else v[:, 0] if k == "surrogates" else v[0] for k, v in stats.items()}
        t = self.time
        return _Coupling(out["mvl"], out["vector"], out["amplitude"], f_phase, f[amp_rows[0]:amp_rows[0] + amp_rows[1]],
                         None if t is None else np.asarray(t)[::window], window, stats)

    def triggered(self, events, *, before, after, freq_limits=None):
        """Event-locked time-frequency averages of the last transform -- the peri-event spectrogram, the evoked
        (phase-locked) part and the inter-trial phase coherence --, reduced on the device over the events.  The
        transform must have been ``output='complex'`` on one device.  ``events``: 1-D event times in seconds on the
        clock of ``time`` (ripples, stimuli, licks, theta troughs; any order, the order given is the order of the
        float32 sums); ``before``, ``after``: seconds >= 0 around each event, nb = round(before fs / K) columns and na
        likewise with the output stride K; ``freq_limits=(lo, hi)``: only the rows whose frequency lies in the closed
        interval (default: all rows).  An event is dropped when it lies in a gap between epochs or outside the
        recording, when its window leaves the recording, or when its window would splice two epochs
        (engine.trigger_columns).  With w_k the coefficient at a lag of event k, E events used and L = nb + na + 1
        lags, the returned object has ``amplitude`` (C, S', L) float32 = mean |w_k| and ``power`` = mean |w_k|^2 (the
        peri-event spectrogram, ERSP), ``evoked`` (C, S', L) complex64 = mean w_k (what is phase-locked to the events),
        ``vector`` (C, S', L) complex64 = mean w_k / |w_k| (its angle: the mean phase), ``itpc`` (C, S', L) float32 =
        |sum w_k / |w_k|| / E in [0, 1], ``lags`` (L,) seconds = arange(-nb, na + 1) K / fs, ``frequencies`` (S',),
        ``events_used`` (a bool mask over ``events``) and ``n_events`` = E; after the reference's single-channel call
        the channel axis is dropped.  The ITPC of E independent phases reads about 0.89 / sqrt(E), not 0 -- a property
        of the estimator, not an error; no surrogate statistics are made.  A baseline ratio (ERSP in dB) is one NumPy
        line on the returned arrays: ``10 * np.log10(r.power / r.power[..., r.lags < -0.05].mean(-1, keepdims=True))``.
        Only the reduced arrays cross to the host; the resident result, ``fetch()`` and the result attributes are
        untouched."""
        from .. import engine
        result, squeeze = self._resident_rows("triggered")
        f = np.array(self._frequencies)
        rows = (0, f.size) if freq_limits is None else engine.coupling_rows(freq_limits, f, "freq_limits")
        stride, fs = self._stride, float(self._fs)
        cols, used, nb, na, why = engine._trigger_scan(events, self.time, fs, stride, before, after, result.shape[2])
        if cols.size == 0:
            raise ValueError("triggered(): none of the %d events can be used: %d lie in a gap between epochs or outside "
                             "the recording, %d have a window (%d columns before, %d after) that leaves the recording, "
                             "%d have a window that would splice two epochs"
                             % (used.size, why["gap"], why["edge"], nb, na, why["splice"]))
        out = _fetched(engine.triggered(result, cols, nb, na, rows), squeeze)
        return _Triggered(out["amplitude"], out["power"], out["evoked"], out["vector"], out["itpc"],
                          np.arange(-nb, na + 1) * stride / fs, f[rows[0]:rows[0] + rows[1]], used, int(cols.size))

    def bandpass(self, bands, *, outputs=("analytic", "envelope", "power")):
        """Band-limited analytic signals of the last transform -- the theta-band trace whose angle is the theta phase
        at every sample, the ripple-band envelope and power at full time resolution --, summed on the device along
        the scale axis: the inverse transform restricted to a band.  The transform must have been
        ``output='complex'`` on one device.  ``bands``: one (f_lo, f_hi) pair in Hz or a sequence of B of them; a band
        holds the rows whose frequency lies in the closed interval, and bands may overlap.  ``outputs``: which of
        'analytic', 'envelope', 'power' to compute.  With w_r the coefficient of row r at a column, the rows of a band
        taken in ascending order and (g, h) = engine.band_weights(frequencies, wavelet), the returned object has
        ``analytic`` (C, B, N) complex64 = sum g_r w_r, ``envelope`` (C, B, N) float32 = |analytic| and ``power``
        (C, B, N) float32 = sum h_r |w_r|^2 (those not asked for are None), ``bands`` (B, 2) as given, ``rows`` (B, 2)
        of (first, count), ``frequencies``: a list of B arrays, and ``time`` (N,): the columns' times (with an output
        stride K, column j is sample K j); after the reference's single-channel call the channel axis is dropped, the
        band axis always stays.  Every sum is a chain of single float32 fused multiply-adds along the band's rows
        (include/ghostcwt.h: gcwt_bandpass): a band has the same bits alone and among any others, and columns in a gap
        between epochs are exactly 0.  The weights are d_r, the cell of row r in ln f, over the integral of the
        wavelet's response (and of its square for ``power``), so a sinusoid of amplitude A well inside a band that
        spans the wavelet's response reads envelope = A and power = A^2 (within 1 % at 4 or more voices per octave).
        A band narrower than the wavelet's own response reads low -- Morse(3, 2) over two octaves reads 0.79 -- a
        property of the wavelet, not an error.  The rows carry each scale's sub-sample delay (even-length kernels in
        'same' mode) and the phase of ``analytic`` inherits it: about 0.25 rad at 80 Hz and 1 kHz.  The phase is one
        NumPy line on the returned array: ``np.angle(r.analytic)``.  Only the band traces cross to the host; the
        resident result, ``fetch()`` and the result attributes are untouched."""
        from .. import engine
        result, squeeze = self._resident_rows("bandpass")
        f = np.array(self._frequencies)
        rows = engine.band_rows(bands, f)
        g, h = engine.band_weights(f, self._wavelet)
        out = _fetched(engine.bandpass(result, rows, g, h, outputs), squeeze)
        t = self.time
        return _Bandpass(out.get("analytic"), out.get("envelope"), out.get("power"),
                         np.asarray(bands, dtype=np.float64).reshape(-1, 2), rows.astype(np.int64),
                         [f[a:a + n] for a, n in rows], None if t is None else np.asarray(t))

    def ridge(self, bands, *, outputs=("row", "amplitude", "frequency", "offset")):
        """The spectral ridge of the last transform inside each band and the instantaneous frequency on it -- at which
        frequency the rhythm is right now and how strong it is there: theta frequency against running speed, the drift
        of a spindle, the chirp inside a ripple --, found on the device.  The transform must have been
        ``output='complex'`` on one device.  ``bands``: one (f_lo, f_hi) pair in Hz or a sequence of B of them, resolved
        as ``bandpass()`` resolves them; bands may overlap.  ``outputs``: which of 'row', 'amplitude', 'frequency',
        'offset' to compute.  With w_r the coefficient of row r at a column, q_r = e_r |w_r|^2 and e =
        engine.ridge_weights(frequencies, wavelet), the returned object has ``row`` (C, B, N) int32: the row of the
        largest q_r among the band's rows, the lowest index among equal ones, and -1 where all are 0 (a gap between
        epochs); ``amplitude`` (C, B, N) float32 = sqrt(q) there (0 in a gap): e makes a sinusoid of amplitude A on a
        row's frequency read A, which for an energy-normalised Morlet transform also keeps the ridge from leaning to
        low frequencies; ``offset`` (C, B, N) float32: the parabolic sub-row position of the maximum of q through the
        winner's two neighbours, in rows, inside [-0.5, 0.5], exactly 0 on a band's first and last row and in a gap;
        ``frequency`` (C, B, N) float32, Hz: the phase advance on the winning row from the column before to the
        column after -- inside the column's own epoch (engine.segments_of), one-sided at its ends --, unwrapped
        against the row's own frequency, so that an output stride K does not alias it; NaN in a gap and in an epoch
        of one column.  Those not asked for are None.  Also ``bands`` (B, 2) as given, ``rows`` (B, 2) of (first,
        count), ``frequencies``: a list of B arrays, ``time`` (N,), and ``grid_frequency()``: ln f of the grid
        interpolated at row + offset, on the host and on request, NaN in a gap.  After the reference's single-channel
        call the channel axis is dropped, the band axis always stays.  ``row``, ``amplitude`` and ``offset`` are
        prescribed single float32 operations and ``frequency`` all but its arctangent (include/ghostcwt.h:
        gcwt_ridge): a band has the same bits alone and among any others.  What the ridge does not do: there is no
        chaining across columns -- every column is ranked on its own --; there is one maximum per band, so two rhythms
        in one band need two bands; and where the two largest rows are nearly equal, ``row`` (with ``offset`` and
        ``grid_frequency()``) flickers between them while ``frequency`` does not.  Only the ridge crosses to the host;
        the resident result, ``fetch()`` and the result attributes are untouched."""
        from .. import engine
        result, squeeze = self._resident_rows("ridge")
        f = np.array(self._frequencies)
        rows = engine.band_rows(bands, f)
        t, nu, hz_per_cycle, segments = self._phase_clock(f, result.shape[2])
        out = _fetched(engine.ridge(result, rows, engine.ridge_weights(f, self._wavelet), nu, hz_per_cycle, segments, outputs),
                       squeeze)
        return _Ridge(out.get("row"), out.get("amplitude"), out.get("frequency"), out.get("offset"),
                      np.asarray(bands, dtype=np.float64).reshape(-1, 2), rows.astype(np.int64),
                      [f[a:a + n] for a, n in rows], t, f)

    def squeeze(self, bins=None, *, freq_limits=None, min_amplitude=0.0, outputs=("coefficients",)):
        """The synchrosqueezed transform of the last transform -- a drifting theta, the chirp inside a ripple or two
        nearby rhythms, sharp in frequency where the rows themselves are an octave wide --, made on the device: every
        coefficient is moved to the frequency cell that its own phase advance names, and what lands in a cell is
        added.  The transform must have been ``output='complex'`` on one device.  ``freq_limits=(lo, hi)``: only the
        rows whose frequency lies in the closed interval are squeezed (default: all rows).  ``bins``: the cells, by
        their centre frequencies: None -- the selected rows' own frequencies (at least 2 rows); an int L >= 2 --
        ``np.geomspace`` between the selected rows' first and last frequency, in the rows' order; an array -- the
        centres themselves, positive and strictly monotonic, at least 2.  The cells' edges are the geometric midpoints
        between neighbouring centres, the outer two half a step beyond (engine.squeeze_edges).  ``min_amplitude``: an
        entry stays out unless its amplitude, in ``ridge().amplitude``'s units (a sinusoid of amplitude A on a row's
        frequency reads A), is above it.  ``outputs``: which of 'coefficients', 'power', 'frequency', 'index' to
        compute.  With w_r the coefficient of row r at a column, g = engine.band_weights(frequencies, wavelet)[0] and
        R selected rows, the returned object has ``frequency`` (C, R, N) float32, Hz: ``ridge()``'s instantaneous
        frequency on every row -- the phase advance from the column before to the column after inside the column's
        own epoch, unwrapped against the row's own frequency, so that an output stride does not alias it; NaN in a gap
        and in an epoch of one column; ``index`` (C, R, N) int32: the cell, as an index into ``bin_frequencies``,
        that the entry was added to, -1 where it stays out: below ``min_amplitude``, no frequency, or a frequency
        outside the cells; ``coefficients`` (C, L, N) complex64: per cell the sum of g_r w_r over its entries, the rows
        in ascending order (one chain of float32 fused multiply-adds per cell and column, ``bandpass()``'s arithmetic:
        the sum over the cells of a column is the analytic signal of the entries that are in); ``power`` (C, L, N)
        float32 = |coefficients|^2.  Those not asked for are None.  Also ``bin_frequencies`` (L,) float64,
        ``edges`` (L + 1,) float32 ascending, ``rows`` = (first, count), ``frequencies`` (R,), ``time`` (N,) and
        ``min_amplitude``.  After the reference's single-channel call the channel axis is dropped.  Columns in a gap
        between epochs are exactly 0 with ``index`` -1.  Everything but the arctangent is prescribed single float32
        operations (include/ghostcwt.h: gcwt_squeeze), without atomics: two runs agree in bits, whichever outputs are
        asked for.  What it does not do: there is no second-order (chirp-rate) correction, so a fast chirp is as
        sharp as its frequency changes little over one wavelet; weak entries carry noise phases and go where those
        say, so on real recordings ``min_amplitude`` is not optional; and the output is as large as the rows it came
        from -- L cells of N columns -- and crosses to the host: fewer cells, fewer outputs or an ``output_stride``
        keep it small.  The resident result, ``fetch()`` and the result attributes are untouched."""
        from .. import engine
        result, squeeze = self._resident_rows("squeeze")
        f = np.array(self._frequencies)
        rows = (0, f.size) if freq_limits is None else engine.coupling_rows(freq_limits, f, "freq_limits")
        own = f[rows[0]:rows[0] + rows[1]]
        if not engine._is_number(min_amplitude) or not np.isfinite(float(min_amplitude)) or float(min_amplitude) < 0:
            raise ValueError("squeeze(): 'min_amplitude' must be a finite number, at least 0, not %r" % (min_amplitude,))
        if bins is None or (isinstance(bins, (int, np.integer)) and not isinstance(bins, (bool, np.bool_))):
            if own.size < 2:
                raise ValueError("squeeze(): bins=%r needs at least 2 selected rows to take the cells from, not %d"
                                 % (bins, own.size))
            if bins is not None and int(bins) < 2:
                raise ValueError("squeeze(): 'bins' must be None, an int >= 2 or an array of centre frequencies, not %r" % (bins,))
            centres = own.astype(np.float64) if bins is None else np.geomspace(own[0], own[-1], int(bins))
        else:
            try:
                centres = np.asarray(bins, dtype=np.float64).ravel()
                ok = np.ndim(bins) == 1 and not isinstance(bins, (str, bytes)) and np.asarray(bins).dtype != np.bool_
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError("squeeze(): 'bins' must be None, an int >= 2 or an array of centre frequencies, not %r" % (bins,))
        edges, descending = engine.squeeze_edges(centres)
        e = engine.ridge_weights(f, self._wavelet).astype(np.float64)
        with np.errstate(over="ignore"):
            floor2 = (np.square(np.float64(min_amplitude)) / e).astype(np.float32)
        if not np.all(np.isfinite(floor2)):
            raise ValueError("squeeze(): 'min_amplitude' = %r squared leaves float32's range" % (min_amplitude,))
        t, nu, hz_per_cycle, segments = self._phase_clock(f, result.shape[2])
        out = _fetched(engine.squeeze(result, rows, engine.band_weights(f, self._wavelet)[0], floor2, nu, hz_per_cycle, segments,
                                      edges, descending, outputs), squeeze)
        return _Squeeze(out.get("coefficients"), out.get("power"), out.get("frequency"), out.get("index"), centres, edges,
                        (int(rows[0]), int(rows[1])), own, t, float(min_amplitude))

    def detect(self, band, *, on="envelope", threshold=3.0, edge=0.0, units="sd", min_duration=0.0, max_duration=None,
               min_gap=0.0, stats="mean", baseline=None, smooth=None, combine=False):
        """Threshold-crossing events of one band of the last transform -- ripples, spindles, bursts: the times that
        ``triggered()`` takes --, found on the device.  The transform must have been ``output='complex'`` on one
        device.  ``band``: one (f_lo, f_hi) pair in Hz, its rows and weights those of ``bandpass()``; ``on``:
        'envelope' or 'power', the band trace of ``bandpass()`` that is thresholded.  The trace stays on the device:
        per channel its mean and sd over the columns that are not exactly 0 (the gaps between epochs) are taken there,
        then the maximal runs of columns with trace > lo and the largest value of each (include/ghostcwt.h:
        gcwt_trace_stats, gcwt_trace_runs), and only those runs cross to the host, 28 bytes each.  ``units='sd'``: hi
        = mean + ``threshold`` sd and lo = mean + ``edge`` sd per channel; ``units='absolute'``: hi = ``threshold``
        and lo = ``edge`` in the trace's units; both rounded to float32 once, and finite hi >= lo >= 0 is required
        (lo >= 0 is what makes the exact zeros of a gap split runs).  An event is a run whose peak is > hi (the double
        threshold: lo sets its boundaries, hi decides); then neighbours in a channel less than ``min_gap`` seconds
        apart -- from the last column of one to the first of the next on the clock of ``time``, so a gap between
        epochs counts with its real length -- are merged, and events shorter than ``min_duration`` or longer than
        ``max_duration`` seconds (columns x K / fs with the output stride K) are dropped (engine.event_filter).  The
        returned object has flat arrays over the events, ordered by channel and then by time: ``channel``, ``start``
        and ``stop`` (seconds: the times of the first and of the last column above lo), ``peak_time``, ``peak``
        (float32: the trace's value there, the first of equal ones), ``start_col``, ``stop_col`` (one past the last
        column) and ``peak_col``; per channel ``mean``, ``sd`` (float64), ``lo``, ``hi`` (float32: the values
        compared with), ``n_columns`` (the non-zero columns) and ``n_candidates`` (the runs above lo, before any
        filtering); and ``band``, ``rows`` (first, count), ``frequencies`` and ``on``.  After the reference's
        single-channel call the per-channel items lose their axis.  ``r.peak_time[r.channel == c]`` is what
        ``triggered()`` takes.  The runs and their peaks are exact, so the events are those of the same definition
        applied to ``bandpass()``'s trace on the host, bit for bit.  The resident result, ``fetch()`` and the result
        attributes are untouched.

        ``smooth``: the standard deviation, in seconds, of a Gaussian that the band trace is smoothed with on the device
        before anything else looks at it (4 ms is usual for ripples): sd_cols = ``smooth`` fs / K columns, cut at half =
        int(4 sd_cols + 0.5) columns to either side as scipy.ndimage.gaussian_filter1d cuts it, the weights normalised
        to sum 1 (engine.smooth_taps; include/ghostcwt.h: gcwt_trace_smooth has the order of the float32 operations).
        The statistics of either kind, ``baseline`` and the runs are then all taken on the smoothed trace, so ``peak``
        is its value.  Every epoch -- a stretch of columns one period apart on the clock of ``time``
        (engine.segments_of) -- is smoothed on its own and continued with zeros past its ends, matching the rows' own
        'same'-mode edges: the trace reads low within 4 sd of an epoch's ends and nothing leaks from one epoch into
        the next.  A ``smooth`` narrower than a column (half = 0) or wider than 4096 columns to either side is refused.
        ``combine=True``: the channels' band traces are averaged on the device, channel 0 first, into one consensus
        trace (the mean over tetrodes that ripples are usually detected on), which is smoothed if ``smooth`` says so
        and then takes the place of the channels: one event list, every ``channel`` -1, and the per-channel items lose
        their axis as after the single-channel call -- after which ``combine`` is refused.  The returned object says
        what was done in ``smooth`` (seconds or None), ``half`` (columns; 0 without smoothing) and ``combined``.  The
        defaults launch what the call launched without them.

        ``stats='median'``: with ``units='sd'`` the centre is the channel's median and the spread 1.482602218505602 x
        its median absolute deviation, the sd of a normal distribution with that MAD -- hi = centre + ``threshold``
        spread, lo = centre + ``edge`` spread, rounded to float32 once -- so the events themselves do not raise the
        thresholds.  Both are exact order statistics of the trace's non-zero columns, selected on the device
        (include/ghostcwt.h: gcwt_trace_order; engine.trace_median_mad has the arithmetic), the bits a sort on the host
        would give, and the per-channel items gain ``median`` and ``mad`` (float64); ``mean`` and ``sd`` are reported
        as before.  With ``units='absolute'`` it is accepted and changes no threshold.  ``baseline=(t0, t1)``: the
        statistics of either kind are taken over the columns with t0 <= time < t1 alone -- seconds on the clock of
        ``time``, or column x K / fs where there are no timestamps -- a quiet stretch; the thresholds hold everywhere
        and the runs are found over the whole trace.  The columns must be one stretch [c0, c1), reported as
        ``baseline_cols``; ``n_columns`` then counts the non-zero columns among them."""
        from .. import engine
        result, squeeze = self._resident_rows("detect")
        if not isinstance(on, str) or on not in ("envelope", "power"):
            raise ValueError("detect(): 'on' must be 'envelope' or 'power', not %r" % (on,))
        if not isinstance(units, str) or units not in ("sd", "absolute"):
            raise ValueError("detect(): 'units' must be 'sd' or 'absolute', not %r" % (units,))
        if not isinstance(stats, str) or stats not in ("mean", "median"):
            raise ValueError("detect(): 'stats' must be 'mean' or 'median', not %r" % (stats,))
        if not isinstance(combine, (bool, np.bool_)):
            raise ValueError("detect(): 'combine' must be True or False, not %r" % (combine,))
        combine = bool(combine)
        if combine and squeeze:
            raise ValueError("detect(): 'combine' averages the channels of a multichannel transform: the last one was the "
                             "single-channel call")
        taps = None
        if smooth is not None:
            if not engine._is_number(smooth) or not np.isfinite(float(smooth)) or float(smooth) <= 0:
                raise ValueError("detect(): 'smooth' must be None or a finite number of seconds > 0, not %r" % (smooth,))
            smooth = float(smooth)
            try:
                taps = engine.smooth_taps(smooth * float(self._fs) / self._stride)
            except ValueError as e:
                raise ValueError("detect(): 'smooth' = %g s at %g columns per second: %s" % (smooth, float(self._fs) / self._stride, e)) from None
        for name, v in (("threshold", threshold), ("edge", edge)):
            if not engine._is_number(v) or not np.isfinite(float(v)):
                raise ValueError("detect(): '%s' must be a finite number, not %r" % (name, v))
        threshold, edge = float(threshold), float(edge)
        if threshold < edge:
            raise ValueError("detect(): hi < lo: 'threshold' (%g) is below 'edge' (%g)" % (threshold, edge))
        if units == "absolute":
            with np.errstate(over="ignore"):
                hi1, lo1 = np.float32(threshold), np.float32(edge)
            if not np.isfinite(hi1):
                raise ValueError("detect(): hi = %g is not finite in float32" % threshold)
            if lo1 < 0:
                raise ValueError("detect(): lo < 0: 'edge' (%g) must be at least 0, the value of a gap between epochs" % edge)
        min_gap, min_duration = engine._seconds(min_gap, "min_gap"), engine._seconds(min_duration, "min_duration")
        max_duration = None if max_duration is None else engine._seconds(max_duration, "max_duration")
        f = np.array(self._frequencies)
        rows = engine.band_rows(band, f)
        if len(rows) != 1:
            raise ValueError("detect() takes one band, (f_lo, f_hi) in Hz, not %d" % len(rows))
        g, h = engine.band_weights(f, self._wavelet)
        t = self.time
        t = None if t is None else np.asarray(t, dtype=np.float64)
        period = self._stride / float(self._fs)
        c0, c1 = 0, int(result.shape[2])
        segments = None
        if taps is not None or combine:
            segments = engine.segments_of(t, period, float(self._fs), c1)     # (c1: every column, before the baseline)
        if baseline is not None:
            c0, c1 = _baseline_columns(baseline, t, c1, period)
        res = engine.bandpass(result, rows, g, h, (on,))
        smoothed = None
        try:
            c, n, pitch = res.n_channels, res.n_cols, res.pitch
            trace = res.buffer.ptr.value + res._offsets()[on]
            if segments is not None:
                # the band trace is replaced by its smoothed (and combined) twin and goes at once
                smoothed, pitch, (c, _) = engine.trace_smooth(trace, pitch, c, n, np.ones(1, np.float32) if taps is None else taps,
                                                              segments, np.arange(c) if combine else None)
                res.free()
                trace = smoothed.ptr.value
            count, mean, sd = engine.trace_stats(trace + 4 * c0, pitch, c, c1 - c0)
            centre, spread = mean, sd
            if stats == "median":
                _, median, mad = engine.trace_median_mad(trace + 4 * c0, pitch, c, c1 - c0)
                centre, spread = median, engine.MAD_TO_SD * mad
            if units == "sd":
                with np.errstate(all="ignore"):
                    hi, lo = (centre + threshold * spread).astype(np.float32), (centre + edge * spread).astype(np.float32)
            else:
                hi, lo = np.full(c, hi1, np.float32), np.full(c, lo1, np.float32)
            bad = np.flatnonzero(~(np.isfinite(hi) & np.isfinite(lo) & (hi >= lo) & (lo >= 0)))
            if bad.size:
                raise ValueError("detect(): channel %d: finite hi >= lo >= 0 is required, not hi = %g and lo = %g (the trace's "
                                 "%s %g, %s %g)" % (bad[0], hi[bad[0]], lo[bad[0]], "mean" if stats == "mean" else "median",
                                                    centre[bad[0]], "sd" if stats == "mean" else "1.4826 MAD", spread[bad[0]]))
            runs = engine.trace_runs(trace, pitch, c, n, lo)
        finally:
            res.free()
            if smoothed is not None:
                smoothed.free()
        ev = engine.event_filter(runs["trace"], runs["start"], runs["stop"], runs["peak_col"], runs["peak"], hi, t, min_gap,
                                 min_duration, max_duration, period)
        when = (lambda col: col * period) if t is None else (lambda col: t[col])
        events = {"channel": np.full_like(ev["trace"], -1) if combine else ev["trace"], "start": when(ev["start"]), "stop": when(ev["stop"] - 1), "peak_time": when(ev["peak_col"]),
                  "peak": ev["peak"], "start_col": ev["start"], "stop_col": ev["stop"], "peak_col": ev["peak_col"]}
        per_channel = {"mean": mean, "sd": sd, "lo": lo, "hi": hi, "n_columns": count, "n_candidates": runs["counts"]}
        if stats == "median":
            per_channel.update(median=median, mad=mad)
        if squeeze or combine:
            per_channel = {k: v[0] for k, v in per_channel.items()}
        if baseline is not None:
            per_channel["baseline_cols"] = (c0, c1)
        first, n_rows = int(rows[0, 0]), int(rows[0, 1])
        f_lo, f_hi = np.asarray(band, dtype=np.float64).ravel()
        return _Events(events, per_channel, (float(f_lo), float(f_hi)), (first, n_rows), f[first:first + n_rows], on,
                       smooth=smooth, half=0 if taps is None else len(taps) - 1, combined=combine)

    def release_device(self):
        """Frees the device copy of the last result (bringing it over first if nothing has asked for it yet)."""
        self._materialize()
        if self._device_result is not None:
            self._device_result.free()
            self._device_result = None

    # -- plotting (reference: transforms.py:233-402) --------------------------
    def plot(self, *, kind=None, timescale=None, logscale=None, standardize=None,
             relative_time=None, center_time=None, time_limits=None, freq_limits=None,
             ax=None, **kwargs):
        """Filled-contour spectrogram; arguments as in the reference."""
        import matplotlib.pyplot as plt

        kind = "amplitude" if kind is None else kind
        if kind not in ("amplitude", "power"):
            raise ValueError("'kind' must be 'amplitude' or 'power', but got {}".format(kind))
        timescale = "seconds" if timescale is None else timescale
        scales = {"milliseconds": (1000.0, "Time (msec)"), "seconds": (1.0, "Time (sec)"),
                  "minutes": (1 / 60.0, "Time (min)"), "hours": (1 / 3600.0, "Time (hr)")}
        if timescale not in scales:
            raise ValueError("timescale must be 'milliseconds', seconds', 'minutes', or "
                             "'hours' but got {}".format(timescale))
        flags = {}
        for name, val, default in (("logscale", logscale, True), ("standardize", standardize, False),
                                   ("relative_time", relative_time, False),
                                   ("center_time", center_time, False)):
            val = default if val is None else val
            if val not in (True, False):
                raise ValueError("'{}' must be True or False but got {}".format(name, val))
            flags[name] = val
        if flags["center_time"] and not flags["relative_time"]:
            raise ValueError("'relative_time' must be True to use option 'center_time'")

        time_slice = slice(None)
        if time_limits is not None:
            if hasattr(time_limits, "data") and not isinstance(time_limits, np.ndarray):
                time_limits = np.asarray(time_limits.data)       # nelpy EpochArray
                if time_limits.shape[0] != 1:
                    raise ValueError("Detected {} epochs but can only restrict spectrogram "
                                     "plot to 1 epoch".format(time_limits.shape[0]))
            elif isinstance(time_limits, (np.ndarray, list)):
                time_limits = np.array(time_limits)
            else:
                raise TypeError("'time_limits' must be of type nelpy.EpochArray or np.ndarray "
                                "but got {}".format(type(time_limits)))
            time_slice = self._restrict_plot_time(time_limits)
        freq_slice = slice(None) if freq_limits is None else self._restrict_plot_freq(freq_limits)

        data = self.amplitude if kind == "amplitude" else self.power
        title = "Wavelet Amplitude Spectrogram" if kind == "amplitude" else "Wavelet Power Spectrogram"
        if data.ndim != 2:
            raise ValueError("plot() shows one channel; index the multichannel result first")
        if flags["standardize"]:
            data = (data - data.mean()) / data.std()
        data = data[freq_slice, time_slice]
        mult, xlabel = scales[timescale]
        timevec = np.array(self.time[time_slice], dtype=np.float64) * mult
        freqvec = self._frequencies[freq_slice]
        if flags["relative_time"]:
            if flags["center_time"]:
                timevec = timevec - timevec[(len(timevec) - 1) // 2]
            else:
                timevec = timevec - timevec[0]
        if ax is None:
            ax = plt.gca()
        tt, ff = np.meshgrid(timevec, freqvec)
        ax.contourf(tt, ff, data, **kwargs)
        if flags["logscale"]:
            ax.set_yscale("log")
        ax.set_title(title)
        ax.set_xlabel(xlabel)
        ax.set_ylabel("Frequency (Hz)")
        return ax

    # -- helpers (reference: transforms.py:404-449) ---------------------------
    def _norm_radians_to_hz(self, val):
        return np.array(val) / np.pi * self._fs / 2.0

    def _hz_to_norm_radians(self, val):
        return np.array(val) / (self._fs / 2.0) * np.pi

    def _check_freq_bounds(self, freq_bounds, freq_bounds_ref):
        lb, ub = freq_bounds
        lb_ref, ub_ref = freq_bounds_ref
        if lb < lb_ref:
            logging.warning("Specified lower bound was {:.3f} Hz but lower bound"
                            " computed on shortest segment was determined"
                            " to be {:.3f} Hz. The lower bound will be adjusted"
                            " upward to {:.3f} Hz accordingly".format(lb, lb_ref, lb_ref))
            lb = lb_ref
        if ub > ub_ref:
            logging.warning("Specified upper bound was {:.3f} Hz but upper bound"
                            " was determined to be {:.3f} Hz. The upper bound"
                            " will be adjusted downward to {:.3f} Hz accordingly"
                            .format(ub, ub_ref, ub_ref))
            ub = ub_ref
        return lb, ub

    def _restrict_plot_time(self, limits):
        limits = np.atleast_1d(np.asarray(limits).squeeze())
        tstart, tstop = np.searchsorted(self.time, limits)
        return slice(tstart, tstop)

    def _restrict_plot_freq(self, limits):
        f0, f1 = np.searchsorted(self._frequencies[::-1], limits)
        return slice(len(self._frequencies) - f1, len(self._frequencies) - f0)

    # -- properties (reference: transforms.py:451-527) ------------------------
    @property
    def fs(self):
        return self._fs

    @fs.setter
    def fs(self, samplerate):
        if samplerate <= 0:
            raise ValueError("Sampling rate must be positive")
        self._fs = samplerate

    @property
    def frequencies(self):
        """The frequencies this transform analyzes, in Hz"""
        return self._frequencies

    @frequencies.setter
    def frequencies(self, val):
        raise ValueError("Setting frequencies outside of cwt() is disallowed. Please use the"
                         " cwt() interface if you want to use a different set of frequencies"
                         " for the cwt")

    @property
    def wavelet(self):
        """Returns wavelet associated with this transform object"""
        return self._wavelet

    @wavelet.setter
    def wavelet(self, wav):
        if not isinstance(wav, wavedef.Wavelet):
            raise TypeError("The wavelet must be of type ghost.Wavelet")
        if wav.fs != self._fs:
            raise ValueError("Wavelet must have same sampling rate as input data")
        self._wavelet = wav

    @property
    def amplitude(self):
        self._materialize()
        if self._amplitude is None:
            if self._power is not None:
                return np.sqrt(self._power)
            if self._coefficients is not None:
                return np.abs(self._coefficients)
        return self._amplitude

    @amplitude.setter
    def amplitude(self, val):
        raise ValueError("Overriding the amplitude attribute is not allowed")

    @property
    def power(self):
        self._materialize()
        if self._power is not None:
            return self._power
        return np.square(self.amplitude)

    @power.setter
    def power(self, val):
        raise ValueError("Overriding the power attribute is not allowed")

    @property
    def coefficients(self):
        """Complex coefficients (only kept when ``output='complex'``)."""
        self._materialize()
        return self._coefficients

    @property
    def time(self):
        if isinstance(self._time, pre.RegularGrid):        # made by the adapter, not asked for until now
            self._time = np.asarray(self._time)
        if self._time_stride > 1 and self._time is not None:   # output_stride: the kept samples' times
            self._time = np.asarray(self._time)[::self._time_stride]
            self._time_stride = 1
        return self._time

    @time.setter
    def time(self, val):
        raise ValueError("Overriding the time attribute is not allowed")
