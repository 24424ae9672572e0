"""G17: Morlet kernels at the ends of the w0 range, and their 'same'-mode convolutions, through the UNMODIFIED
reference (build container only; the reference never travels):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg \
        PYTHONPATH=<reference checkout>:<this repository> python3 tests/golden/make_golden_morlet_w0.py

The recipe of G16 (make_golden_morlet.py) for (w0, fs) in {(2, 1000), (4, 1000), (20, 1000)}: eight frequencies each,
log-spaced across the bounds Morlet.compute_freq_bounds gives for the 4096-sample recording; the reference's
Morlet(w0, freq, fs).get_wavelet(), its length, and fastconv_scipy(x - x.mean(), psi, mode='same') in complex128 on
the columns ``cols`` with each row's largest modulus.  Only inputs and outputs are stored -- no reference code.
"""
import logging
import os

import numpy as np

logging.disable(logging.WARNING)

import ghost as _ref_pkg                                          # refuses the alias package at this repo's root:
HERE = os.path.dirname(os.path.abspath(__file__))
_REPO = os.path.dirname(os.path.dirname(HERE))
assert not os.path.realpath(_ref_pkg.__file__).startswith(os.path.realpath(_REPO) + os.sep), \
    "fixtures must come from the reference: put its checkout FIRST on PYTHONPATH"
from ghost.wave import Morlet                                     # reference
from ghost.sigtools import fastconv_scipy                         # reference

from ghost_amd.synthetic import lfp_channel                       # this repo (workload data)

N = 4096
CASES = [(2.0, 1000.0), (4.0, 1000.0), (20.0, 1000.0)]
N_FREQS = 8


def bounds_hz(w0, fs):
    """The kernel floor(N / 5) samples long; the un-aliased response at Nyquist 0.1 of the peak."""
    kappa = (w0 + np.sqrt(2 + w0 ** 2)) / 2                       # sigma = kappa / omega
    sigma_max = (N // 5 - 1) / 15.0
    sigma_min = (w0 + np.sqrt(2 * np.log(10.0))) / np.pi
    return kappa / sigma_max / (2 * np.pi) * fs, kappa / sigma_min / (2 * np.pi) * fs


def main():
    # the recording's ends (where 'same' mode cuts the kernel) whole, every 8th column between them
    cols = np.unique(np.concatenate([np.arange(256), np.arange(0, N, 8), np.arange(N - 256, N)]))
    arrays = {"cases": np.array(CASES), "n": N, "cols": cols}
    for idx, (w0, fs) in enumerate(CASES):
        x32 = (lfp_channel(N, fs, 32 + idx) * 2.0 - 0.7).astype(np.float32)
        x64 = x32.astype(np.float64)
        lo, hi = bounds_hz(w0, fs)
        freqs = np.geomspace(hi, lo * 1.001, N_FREQS)
        tag = "%g_%g" % (w0, fs)
        arrays["x_" + tag] = x32
        arrays["frequencies_" + tag] = freqs
        lengths = []
        for k, f in enumerate(freqs):
            psi = Morlet(w0=w0, freq=f, fs=fs).get_wavelet()
            lengths.append(len(psi))
            arrays["psi_%s_%d" % (tag, k)] = psi
            conv = fastconv_scipy(x64 - x64.mean(), psi, mode="same").astype(np.complex128)
            arrays["conv_cols_%s_%d" % (tag, k)] = conv[cols]
            arrays["rowmax_%s_%d" % (tag, k)] = np.abs(conv).max()
        arrays["lengths_" + tag] = np.array(lengths)
        print(tag, "freqs", freqs, "lengths", lengths)
    path = os.path.join(HERE, "G17_morlet_w0.npz")
    np.savez_compressed(path, **arrays)
    print("wrote G17_morlet_w0.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
