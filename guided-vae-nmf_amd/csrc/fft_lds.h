// Radix-2 FFT in LDS shared by the power-of-two STFT kernels (aux.hip) and the Bluestein convolution (fft.hip).
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ int bitrev(int x, int bits) { return (int)(__brev((unsigned)x) >> (32 - bits)); }

// in-place complex FFT of length n (power of two) on LDS arrays; sign = -1 forward, +1 inverse
__device__ void fft_lds(double* re, double* im, const double* twr, const double* twi, int n, int bits, int sign) {
  for (int len = 2, st = n >> 1, lh = 0; len <= n; len <<= 1, st >>= 1, ++lh) {
    const int half = len >> 1;                     // = 1 << lh
    for (int b = threadIdx.x; b < (n >> 1); b += blockDim.x) {
      const int grp = b >> lh, pos = b & (half - 1);
      const int i0 = grp * len + pos, i1 = i0 + half;
      const double wr = twr[pos * st], wi = sign * twi[pos * st];
      const double xr = re[i1] * wr - im[i1] * wi, xi = re[i1] * wi + im[i1] * wr;
      re[i1] = re[i0] - xr; im[i1] = im[i0] - xi;
      re[i0] += xr;         im[i0] += xi;
    }
    __syncthreads();
  }
}

}  // namespace
