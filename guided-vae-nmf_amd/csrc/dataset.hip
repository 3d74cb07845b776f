// Noisy data sets on the device: the mixing recipe of the reference's scripts/create_test_set.py:80-103 (joint_norm = 1) and
// scripts/create_noisy_train_set.py:219-250 (joint_norm = 0) for ragged batches, and the per-bin running sums behind
// trainset_mean / trainset_std (create_noisy_train_set.py:299-303).  include/vaenmf.h states the recipe.
//
// Both families are a few bytes of traffic per sample; what they are built for is that an utterance's bits do not depend on
// the batch it sits in or on the run:
//   - the samples of an utterance are cut into nb = min(16, ceil(T' / 4096)) consecutive spans of ceil(T' / nb) samples, one
//     workgroup each: a function of T' alone.  Thread t of a workgroup takes the samples lo + t, lo + t + 256, .. of its span
//     in ascending order, the 64 lanes of a wave are combined by the xor butterfly 32, 16, .. 1, the four waves in wave
//     order, and the workgroup leaves ONE partial.  Every reader of the partials combines them in span order.  No atomics.
//   - every load and store is one float at its natural alignment: rows start wherever the offsets put them (odd lengths
//     leave them 4-byte aligned and no better) and nothing is read outside [cut, T) of a speech row and [b, b + T') of the
//     noise buffer.  A wave still reads 256 consecutive bytes per instruction.
//   - the frames of a spectrogram are cut into nbf = min(256, ceil(n_frames / 64)) spans of ceil(n_frames / nbf) frames (a
//     function of n_frames alone), a workgroup is 64 bins x 4 frame lanes (reads run along the bins), its four lanes are
//     combined in lane order, and a second kernel adds the [nbf][F] partials in span order and then, with accumulate, the
//     total onto the caller's value in one addition.
#include <math.h>
#include <string.h>
#include <vector>
#include "common.h"

namespace {

constexpr int DS_BLOCK = 256;
constexpr int DS_SPAN = 4096;        // samples per workgroup before the cap on workgroups applies
constexpr int DS_MAXB = 16;          // workgroups (and partials) per utterance, at most
constexpr int DS_TAB = 5;            // table rows per utterance: first kept speech sample, T', noise start, output offset, bits of f
constexpr int DS_STATS = 5;          // p, Es, En, k, m
constexpr int DS_CHUNK = 384;        // table entries one ds_put_kernel launch carries (3 KiB of arguments)
constexpr int MO_ROWS = 64;          // frames per workgroup before the cap applies
constexpr int MO_MAXB = 256;         // frame spans, at most
constexpr int MO_COLS = 64;          // bins per workgroup
constexpr int MO_UNROLL = 8;         // frames a thread has in flight
constexpr int MO_FINAL = 16;         // partials of each sum a thread of the final pass has in flight

struct DsChunk { int64_t v[DS_CHUNK]; };

__global__ void ds_put_kernel(DsChunk c, int n, int64_t* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = c.v[i];
}

__host__ __device__ inline int ds_blocks(int64_t T) {
  const int64_t nb = (T + DS_SPAN - 1) / DS_SPAN;
  return nb < 1 ? 1 : (nb > DS_MAXB ? DS_MAXB : (int)nb);
}

// the span of workgroup j of an utterance of T samples: [lo, hi)
__device__ __forceinline__ void ds_span(int64_t T, int j, int64_t& lo, int64_t& hi) {
  const int nb = ds_blocks(T);
  const int64_t span = (T + nb - 1) / nb;
  lo = (int64_t)j * span;
  hi = lo + span < T ? lo + span : T;
  if (lo > T) lo = T;
}

struct DsUtt {
  int64_t a0, T, b, o;     // first kept speech sample, samples kept, first noise sample, first output sample
  double f;
  int nb;
};
__device__ __forceinline__ DsUtt ds_utt(const int64_t* __restrict__ tab, int u) {
  const int64_t* r = tab + (size_t)u * DS_TAB;
  DsUtt d;
  d.a0 = r[0]; d.T = r[1]; d.b = r[2]; d.o = r[3];
  d.f = __builtin_bit_cast(double, r[4]);
  d.nb = ds_blocks(d.T);
  return d;
}

template <bool MAX>
__device__ __forceinline__ double ds_combine(double a, double b) { return MAX ? (a > b ? a : b) : a + b; }

// one value per workgroup in thread 0: lanes by the xor butterfly, waves in wave order
template <bool MAX>
__device__ __forceinline__ double ds_block_reduce(double v, double* red) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v = ds_combine<MAX>(v, __shfl_xor(v, s, 64));
  const int w = threadIdx.x >> 6;
  __syncthreads();                       // red may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double r = red[0];
#pragma unroll
  for (int i = 1; i < DS_BLOCK / 64; ++i) r = ds_combine<MAX>(r, red[i]);
  return r;
}

// p, Es, En, k of an utterance from the partials, combined in span order (every thread of every reader does the same sums)
struct DsGain { double p, Es, En, k, rk; bool ok; };
__device__ __forceinline__ double ds_peak(const double* __restrict__ peakp, int u, int nb) {
  double p = 0.0;
  for (int j = 0; j < nb; ++j) { const double q = peakp[(size_t)u * DS_MAXB + j]; p = q > p ? q : p; }
  return p;
}
__device__ __forceinline__ DsGain ds_gain(const double* __restrict__ peakp, const double* __restrict__ ep, int u, const DsUtt& d) {
  DsGain g;
  g.p = ds_peak(peakp, u, d.nb);
  g.Es = 0.0; g.En = 0.0;
  for (int j = 0; j < d.nb; ++j) {
    g.Es += ep[((size_t)u * DS_MAXB + j) * 2];
    g.En += ep[((size_t)u * DS_MAXB + j) * 2 + 1];
  }
  g.k = 0.0; g.rk = 0.0;
  g.ok = g.p > 0.0 && g.En > 0.0;
  if (g.ok) {
    g.k = g.Es * d.f / g.En;
    g.ok = g.k < INFINITY && g.k == g.k;
    if (!g.ok) g.k = 0.0;
    g.rk = sqrt(g.k);
  }
  return g;
}

// grid: DS_MAXB workgroups per utterance; those past the utterance's own count leave at once
__global__ __launch_bounds__(DS_BLOCK) void mix_peak_kernel(const float* __restrict__ a, const int64_t* __restrict__ tab,
                                                            double* __restrict__ peakp) {
  __shared__ double red[DS_BLOCK / 64];
  const int u = blockIdx.x / DS_MAXB, j = blockIdx.x % DS_MAXB;
  const DsUtt d = ds_utt(tab, u);
  if (j >= d.nb) return;
  int64_t lo, hi;
  ds_span(d.T, j, lo, hi);
  float m = 0.0f;
  for (int64_t i = lo + threadIdx.x; i < hi; i += DS_BLOCK) m = fmaxf(m, fabsf(a[d.a0 + i]));
  const double r = ds_block_reduce<true>((double)m, red);
  if (threadIdx.x == 0) peakp[(size_t)u * DS_MAXB + j] = r;
}

__global__ __launch_bounds__(DS_BLOCK) void mix_energy_kernel(const float* __restrict__ a, const float* __restrict__ noise,
                                                              const int64_t* __restrict__ tab, const double* __restrict__ peakp,
                                                              double* __restrict__ ep) {
  __shared__ double red[DS_BLOCK / 64];
  const int u = blockIdx.x / DS_MAXB, j = blockIdx.x % DS_MAXB;
  const DsUtt d = ds_utt(tab, u);
  if (j >= d.nb) return;
  const double p = ds_peak(peakp, u, d.nb);
  int64_t lo, hi;
  ds_span(d.T, j, lo, hi);
  double es = 0.0, en = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += DS_BLOCK) {
    const double s = p > 0.0 ? (double)a[d.a0 + i] / p : 0.0;
    const double v = (double)noise[d.b + i];
    es += s * s;
    en += v * v;
  }
  es = ds_block_reduce<false>(es, red);
  en = ds_block_reduce<false>(en, red);
  if (threadIdx.x == 0) {
    ep[((size_t)u * DS_MAXB + j) * 2] = es;
    ep[((size_t)u * DS_MAXB + j) * 2 + 1] = en;
  }
}

__global__ __launch_bounds__(DS_BLOCK) void mix_norm_kernel(const float* __restrict__ a, const float* __restrict__ noise,
                                                            const int64_t* __restrict__ tab, const double* __restrict__ peakp,
                                                            const double* __restrict__ ep, double* __restrict__ mp) {
  __shared__ double red[DS_BLOCK / 64];
  const int u = blockIdx.x / DS_MAXB, j = blockIdx.x % DS_MAXB;
  const DsUtt d = ds_utt(tab, u);
  if (j >= d.nb) return;
  const DsGain g = ds_gain(peakp, ep, u, d);
  int64_t lo, hi;
  ds_span(d.T, j, lo, hi);
  double m = 0.0;
  if (g.ok)
    for (int64_t i = lo + threadIdx.x; i < hi; i += DS_BLOCK) {
      const double s = (double)a[d.a0 + i] / g.p, n = g.rk * (double)noise[d.b + i], x = s + n;
      m = fmax(m, fmax(fabs(s), fmax(fabs(n), fabs(x))));
    }
  m = ds_block_reduce<true>(m, red);
  if (threadIdx.x == 0) mp[(size_t)u * DS_MAXB + j] = m;
}

__global__ __launch_bounds__(DS_BLOCK) void mix_write_kernel(const float* __restrict__ a, const float* __restrict__ noise,
                                                             const int64_t* __restrict__ tab, const double* __restrict__ peakp,
                                                             const double* __restrict__ ep, const double* __restrict__ mp,
                                                             int joint_norm, float* __restrict__ so, float* __restrict__ no,
                                                             float* __restrict__ xo, double* __restrict__ stats) {
  const int u = blockIdx.x / DS_MAXB, j = blockIdx.x % DS_MAXB;
  const DsUtt d = ds_utt(tab, u);
  if (j >= d.nb) return;
  const DsGain g = ds_gain(peakp, ep, u, d);
  double m = g.ok ? 1.0 : 0.0;
  if (g.ok && joint_norm) m = ds_peak(mp, u, d.nb);
  if (j == 0 && threadIdx.x == 0) {
    double* st = stats + (size_t)u * DS_STATS;
    st[0] = g.p; st[1] = g.Es; st[2] = g.En; st[3] = g.k; st[4] = m;
  }
  int64_t lo, hi;
  ds_span(d.T, j, lo, hi);
  for (int64_t i = lo + threadIdx.x; i < hi; i += DS_BLOCK) {
    float fs = 0.0f, fn = 0.0f, fx = 0.0f;
    if (g.ok) {
      const double s = (double)a[d.a0 + i] / g.p, n = g.rk * (double)noise[d.b + i], x = s + n;
      fs = (float)(s / m); fn = (float)(n / m); fx = (float)(x / m);
    }
    so[d.o + i] = fs; no[d.o + i] = fn; xo[d.o + i] = fx;
  }
}

// ---- moments ----
__host__ __device__ inline int mo_blocks(int64_t n_frames) {
  const int64_t nb = (n_frames + MO_ROWS - 1) / MO_ROWS;
  return nb > MO_MAXB ? MO_MAXB : (int)nb;
}

// grid (ceil(F / 64), nbf), 256 threads = 64 bins x 4 frame lanes
__global__ __launch_bounds__(DS_BLOCK) void moments_partial_kernel(const float* __restrict__ P, int64_t n_frames, int F, int ld,
                                                                   double* __restrict__ part1, double* __restrict__ part2) {
  __shared__ double r1[4][MO_COLS], r2[4][MO_COLS];
  const int tx = threadIdx.x & (MO_COLS - 1), ty = threadIdx.x / MO_COLS;
  const int f = blockIdx.x * MO_COLS + tx;
  const int nbf = mo_blocks(n_frames);
  const int64_t span = (n_frames + nbf - 1) / nbf;
  const int64_t lo = (int64_t)blockIdx.y * span, hi = lo + span < n_frames ? lo + span : n_frames;
  double s1 = 0.0, s2 = 0.0;
  if (f < F)
    for (int64_t t = lo + ty; t < hi; t += 4 * MO_UNROLL) {      // MO_UNROLL loads in flight, added in frame order
      float v[MO_UNROLL];
#pragma unroll
      for (int i = 0; i < MO_UNROLL; ++i) v[i] = t + 4 * i < hi ? P[(t + 4 * i) * ld + f] : 0.0f;
#pragma unroll
      for (int i = 0; i < MO_UNROLL; ++i)
        if (t + 4 * i < hi) {
          const double d = (double)v[i];
          s1 += d;
          s2 += d * d;
        }
    }
  r1[ty][tx] = s1; r2[ty][tx] = s2;
  __syncthreads();
  if (ty == 0 && f < F) {
    part1[(size_t)blockIdx.y * F + f] = ((r1[0][tx] + r1[1][tx]) + r1[2][tx]) + r1[3][tx];
    part2[(size_t)blockIdx.y * F + f] = ((r2[0][tx] + r2[1][tx]) + r2[2][tx]) + r2[3][tx];
  }
}

__global__ __launch_bounds__(DS_BLOCK) void moments_final_kernel(const double* __restrict__ part1, const double* __restrict__ part2,
                                                                 int nbf, int F, int accumulate, double* __restrict__ S1,
                                                                 double* __restrict__ S2) {
  const int f = blockIdx.x * DS_BLOCK + threadIdx.x;
  if (f >= F) return;
  double s1 = 0.0, s2 = 0.0;
  for (int b = 0; b < nbf; b += MO_FINAL) {               // MO_FINAL loads of each sum in flight, added in span order
    double v1[MO_FINAL], v2[MO_FINAL];
#pragma unroll
    for (int i = 0; i < MO_FINAL; ++i) {
      v1[i] = b + i < nbf ? part1[(size_t)(b + i) * F + f] : 0.0;
      v2[i] = b + i < nbf ? part2[(size_t)(b + i) * F + f] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < MO_FINAL; ++i)
      if (b + i < nbf) { s1 += v1[i]; s2 += v2[i]; }
  }
  S1[f] = accumulate ? S1[f] + s1 : s1;
  S2[f] = accumulate ? S2[f] + s2 : s2;
}

// ---- host ----
struct MixLayout { size_t tab, peakp, ep, mp, total; };
MixLayout mix_layout(int32_t n_utt) {
  MixLayout L;
  size_t p = 0;
  L.tab = p; p += 8 * (size_t)DS_TAB * n_utt;
  L.peakp = p; p += 8 * (size_t)DS_MAXB * n_utt;
  L.ep = p; p += 16 * (size_t)DS_MAXB * n_utt;
  L.mp = p; p += 8 * (size_t)DS_MAXB * n_utt;
  L.total = p;
  return L;
}

template <class T>
T* at(void* work, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(work) + off); }

}  // namespace

extern "C" int64_t vaenmf_mix_work_bytes(int32_t n_utt) {
  if (n_utt < 0 || n_utt > (1 << 24)) {
    vaenmf_set_error("vaenmf_mix_work_bytes: n_utt=%d outside [0, 2^24]", n_utt);
    return -1;
  }
  return (int64_t)mix_layout(n_utt).total;
}

extern "C" int vaenmf_mix_batch(const float* speech, int32_t n_utt, const int64_t* in_offsets, const int64_t* cuts, const float* noise,
                                int64_t noise_len, const int64_t* starts, const double* factors, int32_t joint_norm,
                                const int64_t* out_offsets, float* s, float* n, float* x, double* stats, void* work, int64_t work_bytes,
                                void* stream) {
  VN_REQUIRE(n_utt >= 0 && n_utt <= (1 << 24), "vaenmf_mix_batch: n_utt=%d outside [0, 2^24]", n_utt);
  if (n_utt == 0) return 0;
  VN_REQUIRE(in_offsets && cuts && starts && factors && out_offsets, "vaenmf_mix_batch: null host tables");
  VN_REQUIRE(noise_len >= 0, "vaenmf_mix_batch: noise_len=%lld", (long long)noise_len);
  std::vector<int64_t> tab((size_t)DS_TAB * n_utt);
  for (int32_t u = 0; u < n_utt; ++u) {
    const int64_t T = in_offsets[u + 1] - in_offsets[u], c = cuts[u], b = starts[u];
    VN_REQUIRE(T >= 0, "vaenmf_mix_batch: in_offsets decrease at utterance %d", u);
    VN_REQUIRE(c >= 0, "vaenmf_mix_batch: utterance %d: cut=%lld is negative", u, (long long)c);
    const int64_t Tc = T - c;
    VN_REQUIRE(Tc >= 1, "vaenmf_mix_batch: utterance %d: %lld samples with the first %lld cut leave none", u, (long long)T, (long long)c);
    VN_REQUIRE(b >= 0 && b <= noise_len - Tc, "vaenmf_mix_batch: utterance %d: noise samples [%lld, %lld) leave the buffer of %lld", u,
               (long long)b, (long long)(b + Tc), (long long)noise_len);
    VN_REQUIRE(out_offsets[u + 1] - out_offsets[u] == Tc, "vaenmf_mix_batch: out_offsets give utterance %d %lld samples, it keeps %lld", u,
               (long long)(out_offsets[u + 1] - out_offsets[u]), (long long)Tc);
    VN_REQUIRE(factors[u] > 0.0 && factors[u] < INFINITY, "vaenmf_mix_batch: utterance %d: factor %g is not a positive finite number", u,
               factors[u]);
    int64_t* r = &tab[(size_t)u * DS_TAB];
    r[0] = in_offsets[u] + c; r[1] = Tc; r[2] = b; r[3] = out_offsets[u];
    memcpy(&r[4], &factors[u], 8);
  }
  VN_REQUIRE(in_offsets[0] >= 0 && out_offsets[0] >= 0, "vaenmf_mix_batch: negative first offset");
  const MixLayout L = mix_layout(n_utt);
  VN_REQUIRE(work && ((uintptr_t)work & 7) == 0, "vaenmf_mix_batch: work must be a device buffer aligned to 8 bytes");
  VN_REQUIRE(work_bytes >= (int64_t)L.total, "vaenmf_mix_batch: work_bytes=%lld, vaenmf_mix_work_bytes gives %lld", (long long)work_bytes,
             (long long)L.total);
  VN_REQUIRE(speech && noise && s && n && x && stats, "vaenmf_mix_batch: null buffers");
  VN_REQUIRE(((uintptr_t)stats & 7) == 0, "vaenmf_mix_batch: stats must be aligned to 8 bytes");
  hipStream_t st = (hipStream_t)stream;
  int64_t* d_tab = at<int64_t>(work, L.tab);
  for (size_t i = 0; i < tab.size(); i += DS_CHUNK) {
    DsChunk c;
    const int cnt = (int)(tab.size() - i < (size_t)DS_CHUNK ? tab.size() - i : DS_CHUNK);
    for (int j = 0; j < DS_CHUNK; ++j) c.v[j] = j < cnt ? tab[i + j] : 0;
    hipLaunchKernelGGL(ds_put_kernel, dim3((DS_CHUNK + 127) / 128), dim3(128), 0, st, c, cnt, d_tab + i);
    VN_CHECK_HIP(hipGetLastError());
  }
  double *peakp = at<double>(work, L.peakp), *ep = at<double>(work, L.ep), *mp = at<double>(work, L.mp);
  const dim3 grid((unsigned)n_utt * DS_MAXB), block(DS_BLOCK);
  hipLaunchKernelGGL(mix_peak_kernel, grid, block, 0, st, speech, d_tab, peakp);
  VN_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(mix_energy_kernel, grid, block, 0, st, speech, noise, d_tab, peakp, ep);
  VN_CHECK_HIP(hipGetLastError());
  if (joint_norm) {
    hipLaunchKernelGGL(mix_norm_kernel, grid, block, 0, st, speech, noise, d_tab, peakp, ep, mp);
    VN_CHECK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(mix_write_kernel, grid, block, 0, st, speech, noise, d_tab, peakp, ep, mp, joint_norm != 0, s, n, x, stats);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int64_t vaenmf_moments_work_bytes(int64_t n_frames, int32_t F) {
  if (n_frames < 0 || F < 1) {
    vaenmf_set_error("vaenmf_moments_work_bytes: n_frames=%lld, F=%d", (long long)n_frames, F);
    return -1;
  }
  return (int64_t)16 * mo_blocks(n_frames) * F;
}

extern "C" int vaenmf_feature_moments(const float* P, int64_t n_frames, int32_t F, int32_t ld, int32_t accumulate, double* S1, double* S2,
                                      void* work, int64_t work_bytes, void* stream) {
  VN_REQUIRE(n_frames >= 0 && F >= 1 && ld >= F, "vaenmf_feature_moments: n_frames=%lld, F=%d, ld=%d", (long long)n_frames, F, ld);
  VN_REQUIRE(S1 && S2 && ((uintptr_t)S1 & 7) == 0 && ((uintptr_t)S2 & 7) == 0, "vaenmf_feature_moments: S1 / S2 must be device buffers aligned to 8 bytes");
  const int nbf = mo_blocks(n_frames);
  const int64_t need = (int64_t)16 * nbf * F;
  if (nbf > 0) {
    VN_REQUIRE(P, "vaenmf_feature_moments: null spectrogram");
    VN_REQUIRE(work && ((uintptr_t)work & 7) == 0, "vaenmf_feature_moments: work must be a device buffer aligned to 8 bytes");
    VN_REQUIRE(work_bytes >= need, "vaenmf_feature_moments: work_bytes=%lld, vaenmf_moments_work_bytes gives %lld", (long long)work_bytes,
               (long long)need);
  }
  hipStream_t st = (hipStream_t)stream;
  double* part1 = static_cast<double*>(work);
  double* part2 = nbf > 0 ? part1 + (size_t)nbf * F : nullptr;
  if (nbf > 0) {
    hipLaunchKernelGGL(moments_partial_kernel, dim3((unsigned)((F + MO_COLS - 1) / MO_COLS), (unsigned)nbf), dim3(DS_BLOCK), 0, st, P, n_frames, F,
                       ld, part1, part2);
    VN_CHECK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(moments_final_kernel, dim3((unsigned)((F + DS_BLOCK - 1) / DS_BLOCK)), dim3(DS_BLOCK), 0, st, part1, part2, nbf, F,
                     accumulate != 0, S1, S2);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}
