"""Morlet wavelet object (reference: ghost/wave/morlet.py:10-139).

A time-domain wavelet sampled at ``fs`` with its spectral peak at ``freq`` Hz.  The
reference's ``transform()`` cannot take it (there it is only a kernel factory, with neither
``compute_freq_bounds`` nor ``compute_lengths``); here ``ContinuousWaveletTransform(wavelet=
Morlet(w0=6)).transform(...)`` works like the Morse one: row ``f`` is the 'same'-mode
convolution of the mean-removed recording with ``Morlet(w0, f, fs).get_wavelet()``, made on
the decimated fast path from the kernel's closed-form frequency response.
``w0 < 5`` is not admissible (the zero-mean correction is no longer negligible and the
wavelet answers below zero frequency) but is computed as asked.
"""
import copy

import numpy as np

from .wavelet import Positive, Wavelet

__all__ = ["Morlet"]


class Morlet(Wavelet):

    def __init__(self, *, w0=None, freq=None, fs=None):
        super().__init__()
        self._w0 = 6 if w0 is None else w0          # non-dimensional frequency (> 5: admissible)
        self._freq = 1 if freq is None else freq    # Hz at the spectral peak
        self._fs = 1 if fs is None else fs
        self._scale = None
        self._time_repr = None
        self._recompute()

    def get_wavelet(self):
        return self._time_repr

    def _recompute(self):
        """Scale from the peak frequency (morlet.py:52-54), then the sampled, energy-
        normalised wavelet over 15 scales' worth of samples (morlet.py:56-76)."""
        w0 = self._w0
        self._scale = (w0 + np.sqrt(2 + w0 ** 2)) / (4 * np.pi * self._freq)
        dt = 1 / self._fs
        span = 15 * self._fs * self._scale
        eta = np.arange(-(span + 1) / 2, (span + 1) / 2) * dt / self._scale
        carrier = np.exp(1j * w0 * eta) - np.exp(-0.5 * w0 ** 2)   # zero-mean correction
        self._time_repr = (np.pi ** -0.25 * np.exp(-0.5 * eta ** 2) * carrier
                           * np.sqrt(dt / self._scale))

    # -- what transform() needs of a wavelet (the meaning of Morse's: morse.py:43-55) ----------
    def _samples_per_radian(self):
        """sigma omega: the scale in samples times the analysis frequency in rad / sample."""
        return (self._w0 + np.sqrt(2 + self._w0 ** 2)) / 2

    def compute_freq_bounds(self, N, *, p=None, eta=None):
        """[lowest, highest] analysis frequency (rad/sample) for N samples: the lowest is the one whose
        kernel is floor(N / p) samples long (p = 5: the Morse rule), the highest the one whose un-aliased
        response at the Nyquist frequency is ``eta`` (0.1, morsehigh's criterion) of its peak, i.e. the
        scale of (w0 + sqrt(2 ln(1 / eta))) / pi samples."""
        p = 5 if p is None else p
        eta = 0.1 if eta is None else eta
        sigma_max = (int(np.floor(N / p)) - 1) / 15.0
        sigma_min = (self._w0 + np.sqrt(2 * np.log(1 / eta))) / np.pi
        k = self._samples_per_radian()
        return [k / sigma_max, k / sigma_min]

    def compute_lengths(self, norm_radian_freqs):
        """Kernel length per frequency: exactly ``len(get_wavelet())`` there (the arithmetic of
        ``_recompute``, operation by operation)."""
        freqs = np.atleast_1d(np.asarray(norm_radian_freqs, dtype=np.float64)) / np.pi * self._fs / 2.0
        w0 = self._w0
        scale = (w0 + np.sqrt(2 + w0 ** 2)) / (4 * np.pi * freqs)
        half = (15 * self._fs * scale + 1) / 2
        return np.ceil(half - (-half)).astype(int)

    def copy(self):
        return copy.deepcopy(self)

    # every parameter is positive and re-samples the wavelet when it changes
    fs = Positive("Sampling rate must be positive", after="_changed")
    w0 = Positive("Frequency ratio must be positive", after="_changed")
    freq = Positive("The wavelet frequency must be positive", after="_changed")

    def _changed(self, _value):
        self._recompute()

    @property
    def scale(self):
        return self._scale
