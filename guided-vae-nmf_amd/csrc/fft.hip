// STFT / iSTFT (python/processing/stft.py -> librosa.core.stft / istft) for every n_fft in [16, 4096], fp64 in LDS, one
// workgroup per frame.  The reference's own settings at a power-of-two n_fft <= 2048 run the radix-2 kernels; every other
// length and the options those do not take (any analysis / synthesis window, center=False, constant padding) run one of
// two table-driven FFT plans:
//   * mixed radix (n = 2^a 3^b 5^c 7^d): Stockham autosort stages of radix 4, 2, 3, 5, 7 ping-ponging between two LDS
//     buffers of n complex doubles (32 n bytes, 128 KiB at n = 4096); twiddles exp(-2 pi i t / n) from a global table.
//   * Bluestein (chirp-z, every other n): X[k] = w[k] sum_t (x[t] w[t]) conj(w[k-t]), w[t] = exp(-pi i t^2 / n), as a
//     circular convolution of power-of-two length m >= 2n-1 through the radix-2 fft_lds (16 m bytes of LDS, 128 KiB at
//     m = 8192); the chirp, the m-point twiddles and the spectrum of the conjugate chirp come from global tables.
// Tables are built once per (device, n) on the host in long double, rounded to double and uploaded once.
// Reflect padding follows np.pad(mode="reflect") at any signal length, also when the end-padded signal is shorter than
// the n_fft / 2 samples of padding and the position bounces more than once (reflect_index).
#include <math.h>
#include <map>
#include <mutex>
#include <utility>
#include <vector>
#include "common.h"

namespace {

constexpr int FFT_MIN = 16, FFT_MAX = 4096;

// Device tables of one transform size (pointers into one allocation; unused ones are null)
struct FftPlan {
  int n;                    // transform length
  int m, mbits;             // Bluestein: convolution length and log2; m = 0 for mixed radix
  int nst;                  // mixed radix: number of stages
  uint64_t radix;           // mixed radix: stage radices, 4 bits each, first stage in the low bits
  const double2* tw;        // [n] exp(-2 pi i t / n)                                   (mixed radix)
  const double* hann;       // [n] periodic Hann, the window when the caller passes none
  const double2* chirp;     // [n] exp(-pi i t^2 / n)                                     (Bluestein)
  const double* twr;        // [m/2] cos(-2 pi t / m)                                     (Bluestein)
  const double* twi;        // [m/2] sin(-2 pi t / m)
  const double2* bspec;     // [m] FFT_m(b) / m, b[t] = conj(chirp[|t|]) for |t| < n, circular, zero elsewhere
};

struct FrameArgs {
  int nfft, hop, Fs;
  int center, reflect;
  const double* win;        // [nfft] analysis / synthesis window
};

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// Position p of a signal of Tp samples extended by reflection about its first and last sample, as np.pad(mode="reflect")
// extends it at any length: period 2 (Tp - 1), index 0 when Tp = 1.  One bounce at each end comes first and is all that a
// signal with Tp > n_fft / 2 ever takes; shorter ones fold the position into one period.
__device__ __forceinline__ int64_t reflect_index(int64_t p, int64_t Tp) {
  if (p < 0) p = -p;
  if (p >= Tp) p = 2 * (Tp - 1) - p;
  if (p < 0 || p >= Tp) {
    if (Tp <= 1) return 0;
    const int64_t per = 2 * (Tp - 1);
    p %= per;
    if (p < 0) p += per;
    if (p >= Tp) p = per - p;
  }
  return p;
}

// Sample t of frame i of one utterance: librosa's framing of the end-padded signal (T real samples, Tp after the end pad),
// centre padding by reflection (reflect_index) or with zeros, or no padding at all
__device__ __forceinline__ double frame_sample(const float* __restrict__ wav, int64_t off, int64_t T, int64_t Tp, int i, int t,
                                               const FrameArgs& a) {
  int64_t p = (int64_t)i * a.hop + t - (a.center ? a.nfft / 2 : 0);
  if (a.center && a.reflect) p = reflect_index(p, Tp);
  return (p >= 0 && p < T) ? (double)wav[off + p] : 0.0;
}

// Bin k of the Hermitian extension of a one-sided spectrum row (c2r: the imaginary parts of DC and Nyquist are ignored)
__device__ __forceinline__ double2 hermitian_bin(const float2* __restrict__ row, int k, int nfft) {
  const int half = nfft / 2;
  const float2 v = row[k <= half ? k : nfft - k];
  double vi = k <= half ? (double)v.y : -(double)v.y;
  if (k == 0 || 2 * k == nfft) vi = 0.0;
  return make_double2((double)v.x, vi);
}

// ---------------------------------------------------------------------------------------------------------------------
// Radix-2 FFT in LDS (bitrev, fft_lds: common.h), shared by the power-of-two STFT kernels, the Bluestein convolution and
// the band spectra of stoi.hip
// ---------------------------------------------------------------------------------------------------------------------

// ---------------------------------------------------------------------------------------------------------------------
// Radix-2 path (power-of-two n_fft <= 2048, Hann window, center, reflect padding): radix-2 FFT in LDS, fp64; twiddles and
// window from device sincospi, overlap-add sums in float.  Its output bits differ from the table-driven kernels below.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stft_kernel(const float* __restrict__ wav, const int64_t* __restrict__ samp_off,
                                                   const int32_t* __restrict__ frame_off, const int32_t* __restrict__ frame_utt,
                                                   const int32_t* __restrict__ pad_len, int nfft, int bits, int hop, int Fs,
                                                   float2* __restrict__ X) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* re = reinterpret_cast<double*>(smem);
  double* im = re + nfft;
  double* twr = im + nfft;
  double* twi = twr + nfft / 2;
  const int n = blockIdx.x, u = frame_utt[n], i = n - frame_off[u];
  const int64_t off = samp_off[u];
  const int64_t T = samp_off[u + 1] - off;
  const int64_t Tp = pad_len[u];                 // length after the end-pad rule (stft.py:48-53)
  for (int t = threadIdx.x; t < nfft / 2; t += blockDim.x) {
    double s, c;
    sincospi(-2.0 * t / nfft, &s, &c);           // exp(-2 pi i t / nfft)
    twr[t] = c; twi[t] = s;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < nfft; t += blockDim.x) {
    const int64_t p = reflect_index((int64_t)i * hop + t - nfft / 2, Tp);  // centre=True, reflect padding
    const double v = (p >= 0 && p < T) ? (double)wav[off + p] : 0.0;
    // cos(2 pi t / nfft) from the twiddle table (two thirds of this kernel's time went into a second fp64 sincospi per sample)
    const double cw = t < nfft / 2 ? twr[t] : -twr[t - nfft / 2];
    const int r = bitrev(t, bits);
    re[r] = v * (0.5 - 0.5 * cw);                 // periodic Hann
    im[r] = 0.0;
  }
  __syncthreads();
  fft_lds(re, im, twr, twi, nfft, bits, 1);       // table holds exp(-i..): sign +1 keeps it
  const int F = nfft / 2 + 1;
  for (int f = threadIdx.x; f < Fs; f += blockDim.x)
    X[(size_t)n * Fs + f] = f < F ? make_float2((float)re[f], (float)im[f]) : make_float2(0.f, 0.f);
}

__global__ __launch_bounds__(256) void istft_frames_kernel(const float2* __restrict__ S, int nfft, int bits, int Fs,
                                                           float* __restrict__ work) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* re = reinterpret_cast<double*>(smem);
  double* im = re + nfft;
  double* twr = im + nfft;
  double* twi = twr + nfft / 2;
  const int n = blockIdx.x;
  for (int t = threadIdx.x; t < nfft / 2; t += blockDim.x) {
    double s, c;
    sincospi(2.0 * t / nfft, &s, &c);             // exp(+2 pi i t / nfft)
    twr[t] = c; twi[t] = s;
  }
  const int half = nfft / 2;
  for (int k = threadIdx.x; k < nfft; k += blockDim.x) {
    const int kk = k <= half ? k : nfft - k;
    const float2 v = S[(size_t)n * Fs + kk];
    double vr = v.x, vi = (k <= half) ? v.y : -v.y;
    if (k == 0 || k == half) vi = 0.0;            // c2r ignores the imaginary part of DC / Nyquist
    const int r = bitrev(k, bits);
    re[r] = vr; im[r] = vi;
  }
  __syncthreads();
  fft_lds(re, im, twr, twi, nfft, bits, 1);
  for (int t = threadIdx.x; t < nfft; t += blockDim.x) {
    const double cw = t < nfft / 2 ? twr[t] : -twr[t - nfft / 2];     // cos(2 pi t / nfft), see stft_kernel
    work[(size_t)n * nfft + t] = (float)(re[t] / nfft * (0.5 - 0.5 * cw));
  }
}

__global__ void istft_ola_kernel(const float* __restrict__ work, const int64_t* __restrict__ samp_off,
                                 const int32_t* __restrict__ frame_off, int n_utt, int nfft, int hop,
                                 float* __restrict__ out) {
  const int u = blockIdx.y;
  const int64_t off = samp_off[u], T = samp_off[u + 1] - off;
  const int nb = frame_off[u], nfr = frame_off[u + 1] - nb;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = t + nfft / 2;
    float y = 0.f;
    double wss = 0.0;
    if (p < (int64_t)nfft + (int64_t)hop * (nfr - 1)) {
      int64_t i_lo = (p - nfft + hop) / hop;        // ceil((p - nfft + 1)/hop)
      if (p - nfft + 1 <= 0) i_lo = 0;
      int64_t i_hi = p / hop;
      if (i_hi > nfr - 1) i_hi = nfr - 1;
      for (int64_t i = i_lo; i <= i_hi; ++i) {
        const int tt = (int)(p - i * hop);
        double sw, cw;
        sincospi(2.0 * tt / nfft, &sw, &cw);
        const double wv = 0.5 - 0.5 * cw;
        y += work[(size_t)(nb + i) * nfft + tt];
        wss += wv * wv;
      }
      if (wss > 1.1754943508222875e-38) y = (float)(y / wss);
    }
    out[off + t] = y;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Mixed radix: Stockham stage of radix R.  Ns = product of the radices before this stage; butterfly j reads the R
// points j + r n/R, twiddles them by exp(-2 pi i s r (j mod Ns) / (Ns R)), takes their R-point DFT and writes it to
// (j / Ns) Ns R + (j mod Ns) + r Ns.  s = +1 forward, -1 inverse (unnormalised).
// ---------------------------------------------------------------------------------------------------------------------
template <int R>
__device__ __forceinline__ void dft_small(double2 (&v)[R], const double2 (&root)[R], double s) {
  if constexpr (R == 2) {
    const double2 a = v[0], b = v[1];
    v[0] = make_double2(a.x + b.x, a.y + b.y);
    v[1] = make_double2(a.x - b.x, a.y - b.y);
  } else if constexpr (R == 4) {
    const double2 a = make_double2(v[0].x + v[2].x, v[0].y + v[2].y), b = make_double2(v[0].x - v[2].x, v[0].y - v[2].y);
    const double2 c = make_double2(v[1].x + v[3].x, v[1].y + v[3].y), d = make_double2(v[1].x - v[3].x, v[1].y - v[3].y);
    const double2 wd = make_double2(s * d.y, -s * d.x);                  // exp(-i s pi/2) d
    v[0] = make_double2(a.x + c.x, a.y + c.y);
    v[2] = make_double2(a.x - c.x, a.y - c.y);
    v[1] = make_double2(b.x + wd.x, b.y + wd.y);
    v[3] = make_double2(b.x - wd.x, b.y - wd.y);
  } else {
    double2 y[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      y[q] = v[0];
#pragma unroll
      for (int r = 1; r < R; ++r) {
        const double2 p = cmul(v[r], root[(r * q) % R]);
        y[q].x += p.x; y[q].y += p.y;
      }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) v[q] = y[q];
  }
}

template <int R>
__device__ void mr_stage(const double2* __restrict__ in, double2* __restrict__ out, int n, int Ns, const double2* __restrict__ tw,
                         double s) {
  const int nb = n / R, step = n / (Ns * R);
  double2 root[R];
#pragma unroll
  for (int q = 0; q < R; ++q) { root[q] = tw[q * nb]; root[q].y *= s; }
  for (int j = threadIdx.x; j < nb; j += blockDim.x) {
    const int k = j % Ns;
    double2 v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = in[j + r * nb];
    if (Ns > 1) {
#pragma unroll
      for (int r = 1; r < R; ++r) {
        double2 w = tw[r * k * step];                                    // r k step < R Ns step = n
        w.y *= s;
        v[r] = cmul(v[r], w);
      }
    }
    dft_small<R>(v, root, s);
    const int o = (j - k) * R + k;
#pragma unroll
    for (int r = 0; r < R; ++r) out[o + r * Ns] = v[r];
  }
}

// Whole transform; a holds the input, b is the second buffer.  Returns the buffer that holds the result.
__device__ double2* mr_fft(double2* a, double2* b, const FftPlan& P, double s) {
  int Ns = 1;
  for (int st = 0; st < P.nst; ++st) {
    const int R = (int)((P.radix >> (4 * st)) & 15);
    switch (R) {
      case 2: mr_stage<2>(a, b, P.n, Ns, P.tw, s); break;
      case 3: mr_stage<3>(a, b, P.n, Ns, P.tw, s); break;
      case 4: mr_stage<4>(a, b, P.n, Ns, P.tw, s); break;
      case 5: mr_stage<5>(a, b, P.n, Ns, P.tw, s); break;
      default: mr_stage<7>(a, b, P.n, Ns, P.tw, s); break;
    }
    __syncthreads();
    Ns *= R;
    double2* t = a; a = b; b = t;
  }
  return a;
}

// ---------------------------------------------------------------------------------------------------------------------
// Bluestein: re / im [m] hold x[t] w[t] at bit-reversed positions (zero for t >= n).  Forward m-point FFT, product with
// the conjugate chirp's spectrum written back in bit-reversed order (each thread swaps one pair k <= bitrev(k)),
// inverse m-point FFT: re / im [k] = sum_t x[t] w[t] conj(w[k-t]) for k < n (the 1/m is folded into bspec).
// ---------------------------------------------------------------------------------------------------------------------
__device__ void bs_convolve(double* re, double* im, const FftPlan& P) {
  fft_lds(re, im, P.twr, P.twi, P.m, P.mbits, 1);                  // table holds exp(-i..): sign +1 keeps it
  for (int k = threadIdx.x; k < P.m; k += blockDim.x) {
    const int j = bitrev(k, P.mbits);
    if (k > j) continue;
    const double2 bk = P.bspec[k], bj = P.bspec[j];
    const double2 xk = make_double2(re[k], im[k]), xj = make_double2(re[j], im[j]);
    const double2 pk = cmul(xk, bk), pj = cmul(xj, bj);
    re[j] = pk.x; im[j] = pk.y;
    re[k] = pj.x; im[k] = pj.y;
  }
  __syncthreads();
  fft_lds(re, im, P.twr, P.twi, P.m, P.mbits, -1);
}

// ---------------------------------------------------------------------------------------------------------------------
// Analysis: frame, window, FFT, bins [0, F) to X [NT][Fs] as complex64, bins >= F zeroed
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stft_mr_kernel(const float* __restrict__ wav, const int64_t* __restrict__ samp_off,
                                                      const int32_t* __restrict__ frame_off, const int32_t* __restrict__ frame_utt,
                                                      const int32_t* __restrict__ pad_len, FrameArgs a, FftPlan P,
                                                      float2* __restrict__ X) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double2* A = reinterpret_cast<double2*>(smem);
  double2* B = A + a.nfft;
  const int n = blockIdx.x, u = frame_utt[n], i = n - frame_off[u];
  const int64_t off = samp_off[u], T = samp_off[u + 1] - off, Tp = pad_len[u];
  for (int t = threadIdx.x; t < a.nfft; t += blockDim.x)
    A[t] = make_double2(frame_sample(wav, off, T, Tp, i, t, a) * a.win[t], 0.0);
  __syncthreads();
  const double2* Y = mr_fft(A, B, P, 1.0);
  const int F = a.nfft / 2 + 1;
  for (int f = threadIdx.x; f < a.Fs; f += blockDim.x)
    X[(size_t)n * a.Fs + f] = f < F ? make_float2((float)Y[f].x, (float)Y[f].y) : make_float2(0.f, 0.f);
}

__global__ __launch_bounds__(256) void stft_bs_kernel(const float* __restrict__ wav, const int64_t* __restrict__ samp_off,
                                                      const int32_t* __restrict__ frame_off, const int32_t* __restrict__ frame_utt,
                                                      const int32_t* __restrict__ pad_len, FrameArgs a, FftPlan P,
                                                      float2* __restrict__ X) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* re = reinterpret_cast<double*>(smem);
  double* im = re + P.m;
  const int n = blockIdx.x, u = frame_utt[n], i = n - frame_off[u];
  const int64_t off = samp_off[u], T = samp_off[u + 1] - off, Tp = pad_len[u];
  for (int t = threadIdx.x; t < P.m; t += blockDim.x) {
    const int r = bitrev(t, P.mbits);
    if (t < a.nfft) {
      const double v = frame_sample(wav, off, T, Tp, i, t, a) * a.win[t];
      const double2 c = P.chirp[t];
      re[r] = v * c.x; im[r] = v * c.y;
    } else {
      re[r] = 0.0; im[r] = 0.0;
    }
  }
  __syncthreads();
  bs_convolve(re, im, P);
  const int F = a.nfft / 2 + 1;
  for (int f = threadIdx.x; f < a.Fs; f += blockDim.x) {
    float2 o = make_float2(0.f, 0.f);
    if (f < F) {
      const double2 y = cmul(make_double2(re[f], im[f]), P.chirp[f]);
      o = make_float2((float)y.x, (float)y.y);
    }
    X[(size_t)n * a.Fs + f] = o;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Synthesis, per frame: inverse real FFT of the one-sided row, / n, times the synthesis window -> work [NT][nfft]
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void istft_mr_frames_kernel(const float2* __restrict__ S, FrameArgs a, FftPlan P,
                                                              float* __restrict__ work) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double2* A = reinterpret_cast<double2*>(smem);
  double2* B = A + a.nfft;
  const int n = blockIdx.x;
  const float2* row = S + (size_t)n * a.Fs;
  for (int k = threadIdx.x; k < a.nfft; k += blockDim.x) A[k] = hermitian_bin(row, k, a.nfft);
  __syncthreads();
  const double2* Y = mr_fft(A, B, P, -1.0);
  for (int t = threadIdx.x; t < a.nfft; t += blockDim.x)
    work[(size_t)n * a.nfft + t] = (float)(Y[t].x / a.nfft * a.win[t]);
}

// The inverse DFT as conj(DFT(conj(Y))): only its real part is kept, so the outer conjugation drops out
__global__ __launch_bounds__(256) void istft_bs_frames_kernel(const float2* __restrict__ S, FrameArgs a, FftPlan P,
                                                              float* __restrict__ work) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* re = reinterpret_cast<double*>(smem);
  double* im = re + P.m;
  const int n = blockIdx.x;
  const float2* row = S + (size_t)n * a.Fs;
  for (int t = threadIdx.x; t < P.m; t += blockDim.x) {
    const int r = bitrev(t, P.mbits);
    if (t < a.nfft) {
      const double2 y = hermitian_bin(row, t, a.nfft);
      const double2 v = cmul(make_double2(y.x, -y.y), P.chirp[t]);
      re[r] = v.x; im[r] = v.y;
    } else {
      re[r] = 0.0; im[r] = 0.0;
    }
  }
  __syncthreads();
  bs_convolve(re, im, P);
  for (int t = threadIdx.x; t < a.nfft; t += blockDim.x) {
    const double2 c = P.chirp[t];
    work[(size_t)n * a.nfft + t] = (float)((re[t] * c.x - im[t] * c.y) / a.nfft * a.win[t]);
  }
}

// Overlap-add of the windowed frames, divided by the window's sum of squares where it exceeds float32's tiny (librosa),
// trimmed by n/2 samples when center, zero beyond the last frame; one utterance per blockIdx.y, T = its output length
__global__ void istft_win_ola_kernel(const float* __restrict__ work, const int64_t* __restrict__ samp_off,
                                     const int32_t* __restrict__ frame_off, int nfft, int hop, int center,
                                     const double* __restrict__ win, float* __restrict__ out) {
  const int u = blockIdx.y;
  const int64_t off = samp_off[u], T = samp_off[u + 1] - off;
  const int nb = frame_off[u], nfr = frame_off[u + 1] - nb;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = t + (center ? nfft / 2 : 0);
    double y = 0.0, wss = 0.0;
    if (p < (int64_t)nfft + (int64_t)hop * (nfr - 1)) {
      int64_t i_lo = (p - nfft + hop) / hop;        // ceil((p - nfft + 1)/hop)
      if (p - nfft + 1 <= 0) i_lo = 0;
      int64_t i_hi = p / hop;
      if (i_hi > nfr - 1) i_hi = nfr - 1;
      for (int64_t i = i_lo; i <= i_hi; ++i) {
        const int tt = (int)(p - i * hop);
        y += work[(size_t)(nb + i) * nfft + tt];
        wss += win[tt] * win[tt];
      }
      if (wss > 1.1754943508222875e-38) y /= wss;
    }
    out[off + t] = (float)y;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Host: plans
// ---------------------------------------------------------------------------------------------------------------------
struct PlanEntry {
  FftPlan p;
  void* mem;
};

// radices of n over {4, 2, 3, 5, 7} (at most one 2), packed 4 bits per stage; false if n has a prime factor above 7
bool factor_small(int n, uint64_t* radix, int* nst) {
  uint64_t r = 0;
  int k = 0;
  auto push = [&](int f) { r |= (uint64_t)f << (4 * k); ++k; n /= f; };
  while (n % 4 == 0) push(4);
  if (n % 2 == 0) push(2);
  for (int f : {3, 5, 7})
    while (n % f == 0) push(f);
  *radix = r; *nst = k;
  return n == 1 && k <= 16;
}

// exp(-2 pi i a / b) in long double, rounded once
double2 unit(long long a, long long b) {
  const long double ang = -2.0L * 3.14159265358979323846264338327950288L * (long double)(a % b) / (long double)b;
  return make_double2((double)cosl(ang), (double)sinl(ang));
}

int build_plan(int n, PlanEntry* e) {
  FftPlan& P = e->p;
  P = FftPlan{};
  P.n = n;
  const bool mixed = factor_small(n, &P.radix, &P.nst);
  if (!mixed) {
    P.m = 1; P.mbits = 0;
    while (P.m < 2 * n - 1) { P.m <<= 1; ++P.mbits; }
  }
  const int m = P.m;
  // byte layout: hann [n] | tw [n] or chirp [n] | twr, twi [m/2] | bspec [m]
  const size_t o_hann = 0, o_c = o_hann + 8 * (size_t)n, o_twr = o_c + 16 * (size_t)n, o_twi = o_twr + 4 * (size_t)m,
               o_b = o_twi + 4 * (size_t)m, bytes = o_b + 16 * (size_t)m;
  std::vector<char> h(bytes);
  double* hann = reinterpret_cast<double*>(h.data() + o_hann);
  double2* c = reinterpret_cast<double2*>(h.data() + o_c);
  for (int t = 0; t < n; ++t) hann[t] = 0.5 - 0.5 * unit(t, n).x;
  if (mixed) {
    for (int t = 0; t < n; ++t) c[t] = unit(t, n);
  } else {
    for (int t = 0; t < n; ++t) c[t] = unit((long long)t * t, 2LL * n);   // exp(-pi i t^2 / n), t^2 reduced mod 2n
    double* twr = reinterpret_cast<double*>(h.data() + o_twr);
    double* twi = reinterpret_cast<double*>(h.data() + o_twi);
    for (int t = 0; t < m / 2; ++t) { const double2 w = unit(t, m); twr[t] = w.x; twi[t] = w.y; }
    // spectrum of b (conjugate chirp, circular), long double radix-2 DIT on the host
    std::vector<long double> br(m, 0.0L), bi(m, 0.0L);
    for (int t = 0; t < n; ++t) {
      const long double ang = 3.14159265358979323846264338327950288L * (long double)(((long long)t * t) % (2LL * n)) / n;
      const int pos[2] = {t, (m - t) & (m - 1)};
      for (int q = 0; q < (t ? 2 : 1); ++q) {
        const int r = (int)(__builtin_bitreverse32((unsigned)pos[q]) >> (32 - P.mbits));
        br[r] = cosl(ang); bi[r] = sinl(ang);
      }
    }
    for (int len = 2; len <= m; len <<= 1)
      for (int g = 0; g < m; g += len)
        for (int k = 0; k < len / 2; ++k) {
          const long double ang = -2.0L * 3.14159265358979323846264338327950288L * k / len;
          const long double wr = cosl(ang), wi = sinl(ang);
          const int i0 = g + k, i1 = i0 + len / 2;
          const long double xr = br[i1] * wr - bi[i1] * wi, xi = br[i1] * wi + bi[i1] * wr;
          br[i1] = br[i0] - xr; bi[i1] = bi[i0] - xi;
          br[i0] += xr; bi[i0] += xi;
        }
    double2* bs = reinterpret_cast<double2*>(h.data() + o_b);
    for (int k = 0; k < m; ++k) bs[k] = make_double2((double)(br[k] / m), (double)(bi[k] / m));
  }
  char* d = nullptr;
  VN_CHECK_HIP(hipMalloc(&d, bytes));
  const hipError_t ec = hipMemcpy(d, h.data(), bytes, hipMemcpyHostToDevice);
  if (ec != hipSuccess) {
    (void)hipFree(d);
    VN_CHECK_HIP(ec);
  }
  e->mem = d;
  P.hann = reinterpret_cast<const double*>(d + o_hann);
  if (mixed) {
    P.tw = reinterpret_cast<const double2*>(d + o_c);
  } else {
    P.chirp = reinterpret_cast<const double2*>(d + o_c);
    P.twr = reinterpret_cast<const double*>(d + o_twr);
    P.twi = reinterpret_cast<const double*>(d + o_twi);
    P.bspec = reinterpret_cast<const double2*>(d + o_b);
  }
  return 0;
}

// The plan of size n on the current device, built on first use (one upload) and kept for the life of the process
int get_plan(int n, FftPlan* out) {
  static std::mutex mu;
  static std::map<std::pair<int, int>, PlanEntry> plans;
  int dev = 0;
  VN_CHECK_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  auto it = plans.find({dev, n});
  if (it == plans.end()) {
    PlanEntry e;
    if (int rc = build_plan(n, &e)) return rc;
    it = plans.emplace(std::make_pair(dev, n), e).first;
  }
  *out = it->second.p;
  return 0;
}

size_t frame_lds(const FftPlan& P) { return P.m ? (size_t)16 * P.m : (size_t)32 * P.n; }
size_t r2_lds(int nfft) { return (size_t)nfft * 3 * sizeof(double); }      // radix-2 kernels: re, im, twiddles
int ilog2(int n) { int b = 0; while ((1 << b) < n) ++b; return b; }

// the radix-2 kernels take the reference's own settings at power-of-two lengths
bool radix2_path(const vaenmf_stft_opts* o) {
  return o->nfft <= 2048 && (o->nfft & (o->nfft - 1)) == 0 && o->window == nullptr && o->center && o->pad_mode == VAENMF_PAD_REFLECT;
}

int check_opts(const vaenmf_stft_opts* o, int32_t Fs, const char* who) {
  VN_REQUIRE(o, "%s: null options", who);
  VN_REQUIRE(o->nfft >= FFT_MIN && o->nfft <= FFT_MAX, "%s: n_fft=%d: this build takes window lengths in [%d, %d]", who,
             o->nfft, FFT_MIN, FFT_MAX);
  VN_REQUIRE(o->hop > 0, "%s: hop must be positive", who);
  VN_REQUIRE(o->pad_mode == VAENMF_PAD_REFLECT || o->pad_mode == VAENMF_PAD_CONSTANT, "%s: pad_mode %d not supported", who, o->pad_mode);
  VN_REQUIRE(Fs >= o->nfft / 2 + 1, "%s: Fs=%d < n_fft/2+1", who, Fs);
  return 0;
}

}  // namespace

extern "C" int vaenmf_stft_geometry(int64_t n_samples, double fs, double wlen_sec, double hop_percent, int32_t center,
                                    int32_t* nfft, int32_t* hop, int32_t* n_frames, int32_t* n_padded) {
  VN_REQUIRE(wlen_sec * fs == (double)(int64_t)(wlen_sec * fs), "wlen_sample of STFT is not an integer.");  // stft.py:37-38
  const int nf = (int)(wlen_sec * fs);
  const int hp = (int)(hop_percent * nf);
  VN_REQUIRE(nf >= FFT_MIN && nf <= FFT_MAX, "n_fft=%d: this build takes window lengths in [%d, %d]", nf, FFT_MIN, FFT_MAX);
  VN_REQUIRE(hp > 0, "hop must be positive");
  const double utt_len = (double)n_samples / fs;                                                            // stft.py:49
  const double ratio = utt_len / wlen_sec / hop_percent;
  int64_t Tp = n_samples;
  if (ceil(ratio) != (double)(int64_t)ratio) Tp += hp;                                                      // stft.py:50-51
  int64_t nfr;
  if (center) {
    nfr = 1 + (Tp + 2 * (nf / 2) - nf) / hp;                  // librosa pads n_fft//2 on both sides
  } else {
    VN_REQUIRE(Tp >= nf, "center=False: the signal (%lld samples after the end pad) is shorter than n_fft=%d",
               (long long)Tp, nf);
    nfr = 1 + (Tp - nf) / hp;
  }
  *nfft = nf; *hop = hp; *n_padded = (int32_t)Tp; *n_frames = (int32_t)nfr;
  return 0;
}

extern "C" int vaenmf_stft_batch_ex(const float* wav, int32_t n_frames_total, const int64_t* sample_offsets,
                                    const int32_t* frame_offsets, const int32_t* frame_utt, const int32_t* padded_len,
                                    const vaenmf_stft_opts* opts, int32_t Fs, float* X, void* stream) {
  VN_REQUIRE(wav && X && n_frames_total > 0 && sample_offsets && frame_offsets && frame_utt && padded_len,
             "vaenmf_stft_batch_ex: bad arguments");
  if (int rc = check_opts(opts, Fs, "vaenmf_stft_batch_ex")) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (radix2_path(opts)) {
    hipLaunchKernelGGL(stft_kernel, dim3(n_frames_total), dim3(256), r2_lds(opts->nfft), st, wav, sample_offsets, frame_offsets,
                       frame_utt, padded_len, opts->nfft, ilog2(opts->nfft), opts->hop, Fs, reinterpret_cast<float2*>(X));
    VN_CHECK_HIP(hipGetLastError());
    return 0;
  }
  FftPlan P;
  if (int rc = get_plan(opts->nfft, &P)) return rc;
  const FrameArgs a{opts->nfft, opts->hop, Fs, opts->center ? 1 : 0, opts->pad_mode == VAENMF_PAD_REFLECT ? 1 : 0,
                    opts->window ? opts->window : P.hann};
  const size_t lds = frame_lds(P);
  const void* fn = P.m ? (const void*)stft_bs_kernel : (const void*)stft_mr_kernel;
  if (int e = vn_ensure_dyn_lds(fn, VN_LDS_LIMIT)) return e;
  if (P.m)
    hipLaunchKernelGGL(stft_bs_kernel, dim3(n_frames_total), dim3(256), lds, st, wav, sample_offsets, frame_offsets, frame_utt,
                       padded_len, a, P, reinterpret_cast<float2*>(X));
  else
    hipLaunchKernelGGL(stft_mr_kernel, dim3(n_frames_total), dim3(256), lds, st, wav, sample_offsets, frame_offsets, frame_utt,
                       padded_len, a, P, reinterpret_cast<float2*>(X));
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int vaenmf_istft_batch_ex(const float* S, int32_t n_utt, int32_t n_frames_total, const int64_t* sample_offsets,
                                     const int32_t* frame_offsets, const vaenmf_stft_opts* opts, int32_t Fs, float* work,
                                     float* wav_out, void* stream) {
  VN_REQUIRE(S && work && wav_out && n_utt > 0 && n_frames_total > 0 && sample_offsets && frame_offsets,
             "vaenmf_istft_batch_ex: bad arguments");
  if (int rc = check_opts(opts, Fs, "vaenmf_istft_batch_ex")) return rc;
  hipStream_t st = (hipStream_t)stream;
  const float2* S2 = reinterpret_cast<const float2*>(S);
  if (radix2_path(opts)) {
    hipLaunchKernelGGL(istft_frames_kernel, dim3(n_frames_total), dim3(256), r2_lds(opts->nfft), st, S2, opts->nfft, ilog2(opts->nfft), Fs, work);
    hipLaunchKernelGGL(istft_ola_kernel, dim3(64, n_utt), dim3(256), 0, st, work, sample_offsets, frame_offsets, n_utt, opts->nfft,
                       opts->hop, wav_out);
    VN_CHECK_HIP(hipGetLastError());
    return 0;
  }
  FftPlan P;
  if (int rc = get_plan(opts->nfft, &P)) return rc;
  const FrameArgs a{opts->nfft, opts->hop, Fs, opts->center ? 1 : 0, 0, opts->window ? opts->window : P.hann};
  const size_t lds = frame_lds(P);
  const void* fn = P.m ? (const void*)istft_bs_frames_kernel : (const void*)istft_mr_frames_kernel;
  if (int e = vn_ensure_dyn_lds(fn, VN_LDS_LIMIT)) return e;
  if (P.m)
    hipLaunchKernelGGL(istft_bs_frames_kernel, dim3(n_frames_total), dim3(256), lds, st, S2, a, P, work);
  else
    hipLaunchKernelGGL(istft_mr_frames_kernel, dim3(n_frames_total), dim3(256), lds, st, S2, a, P, work);
  hipLaunchKernelGGL(istft_win_ola_kernel, dim3(64, n_utt), dim3(256), 0, st, work, sample_offsets, frame_offsets, a.nfft, a.hop,
                     a.center, a.win, wav_out);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}
