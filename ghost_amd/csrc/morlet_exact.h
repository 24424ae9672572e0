// morlet_exact.h -- the Morlet kernel of ghost/wave/morlet.py:56-76 and its frequency response in closed
// form (host and device, fp64).
//
// For analysis frequency f the kernel is Morlet(w0, f, fs).get_wavelet():
//   scale = (w0 + sqrt(2 + w0^2)) / (4 pi f),  sigma = scale fs  (the scale in samples),  M = 15 sigma,
//   eta[n] = (n - c0) / sigma,  c0 = (M + 1) / 2,  n = 0 .. L - 1,  L = ceil(M + 1),
//   psi[n] = pi^(-1/4) sigma^(-1/2) exp(-eta^2 / 2) (exp(i w0 eta) - exp(-w0^2 / 2)).
// Its centre eta = 0 lies at c0, which is neither a sample nor half-way between two: against the origin of
// 'same' mode, (L - 1) // 2, the kernel is delayed by d = c0 - (L - 1) // 2, a real number in (0, 1] of its
// own for every scale.  With F(xi) = sqrt(2 pi) (exp(-(xi - w0)^2 / 2) - exp(-w0^2 / 2) exp(-xi^2 / 2)), the
// transform of the continuous wavelet, Poisson's sum gives the response of the sampled kernel in the engine's
// convention H(theta) = sum_n psi[n] exp(-i theta (n - (L-1)//2)):
//
//   H(theta) = pi^(-1/4) sqrt(sigma) sum_k F(sigma theta_k) exp(-i theta_k d),   theta_k = theta + 2 pi k
//
// to 3e-12 of its peak (the kernel is cut at 7.5 sigma, where the Gaussian is e^-28).  Three alias terms
// either side of k = 0 are kept: they matter at the top of a grid only (sigma of a few samples); wherever a
// scale can be decimated the sum is its k = 0 term, real and positive, times the delay's phase.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace gcwt {

struct MorletScale {
  double sigma;      // scale in samples
  double c0;         // array index of the wavelet's centre
  double delay;      // d = c0 - (L - 1) // 2
  int64_t length;    // L
};

// the arithmetic of morlet.py:52-59, operation by operation, so that L is the length of get_wavelet()
__host__ __device__ inline MorletScale morlet_scale(double w0, double freq_hz, double fs) {
  MorletScale m;
  const double scale = (w0 + sqrt(2.0 + w0 * w0)) / (4.0 * M_PI * freq_hz);
  const double span = 15.0 * fs * scale;
  const double half = (span + 1.0) / 2.0;
  m.length = (int64_t)ceil(half - (-half));       // numpy.arange(-half, half): ceil((stop - start) / 1)
  if (m.length < 1) m.length = 1;
  m.sigma = scale * fs;
  m.c0 = half;
  m.delay = half - (double)((m.length - 1) / 2);
  return m;
}

// F(xi) / sqrt(2 pi)
__host__ __device__ inline double morlet_shape(double xi, double w0) {
  return exp(-0.5 * (xi - w0) * (xi - w0)) - exp(-0.5 * w0 * w0 - 0.5 * xi * xi);
}

// pi^(-1/4) sqrt(sigma) sqrt(2 pi): H's factor in front of the sum of shapes
__host__ __device__ inline double morlet_norm(double sigma) { return 1.8827925275534296 * sqrt(sigma); }

// H(2 pi a / b), b > 0, any a (reduced in integers to [-b/2, b/2])
__host__ __device__ inline void morlet_response(double w0, double sigma, double delay, int64_t a, int64_t b,
                                                double* re, double* im) {
  int64_t m = a % b;
  if (m < 0) m += b;
  if (2 * m > b) m -= b;
  const double turns = (double)m / (double)b;      // theta / 2 pi in [-1/2, 1/2]
  double sr = 0.0, si = 0.0;
  for (int k = -3; k <= 3; ++k) {
    const double tk = turns + (double)k;
    const double f = morlet_shape(2.0 * M_PI * tk * sigma, w0);
    double sn, cs;
    sincos(-2.0 * M_PI * tk * delay, &sn, &cs);
    sr += f * cs;
    si += f * sn;
  }
  const double c = morlet_norm(sigma);
  *re = c * sr;
  *im = c * si;
}

// tap n of the literal kernel
__host__ __device__ inline void morlet_tap(double w0, double sigma, double c0, int64_t n, double* re, double* im) {
  const double eta = ((double)n - c0) / sigma;
  const double env = 0.7511255444649425 / sqrt(sigma) * exp(-0.5 * eta * eta);   // pi^(-1/4)
  double sn, cs;
  sincos(w0 * eta, &sn, &cs);
  *re = env * (cs - exp(-0.5 * w0 * w0));
  *im = env * sn;
}

}  // namespace gcwt
