// Small kernels around the hot loop: W multiplicative update, cost reduction,
// dense layers (encoder / classifier), |X|^2, NMF initialisation, SI-SDR Gram sums.
#include "common.h"

typedef __attribute__((ext_vector_type(4))) unsigned u32x4p;

namespace {

// ----------------------------------------------------------------------------
// W update (mcem.py:107-110) + L1 column normalisation (mcem.py:129-133), two stages:
//   w_partial_kernel: num[f,k] = sum_n P[n,f] H[k,n], den[f,k] = sum_n A1[n,f] H[k,n] over one of
//                     NCH frame chunks of an utterance (P = X2 * sum_r Vx^-2, A1 = sum_r Vx^-1 come from
//                     decode_kernel<MODE_WSTATS>); grid (NCH, U), one thread per bin
//   w_update_kernel:  fixed-order sum of the NCH partials, W <- W sqrt(num/den), column norms
// ----------------------------------------------------------------------------
constexpr int W_NCH = 8;

// Ranks are independent in the update (the column norms are per rank): w_update_kernel splits the padded ranks above 8
// over blockIdx.y in groups of KG = 8 -- one workgroup per utterance before, 64 workgroups on 256 CUs; rank 32: 56 -> 21 us.
constexpr int W_KG = 8;

template <int KP>
__global__ __launch_bounds__(640) void w_partial_kernel(const float* __restrict__ A1, const float* __restrict__ P,
                                                        const float* __restrict__ Ht, float* __restrict__ part,
                                                        const int32_t* __restrict__ frame_off, int Fs) {
  // (not split over rank groups: every group would read the A1 / P rows again -- measured 64 -> 71 us at rank 32)
  const int u = blockIdx.y, ch = blockIdx.x, f = threadIdx.x;
  const int nb = frame_off[u], ne = frame_off[u + 1];
  const int per = (ne - nb + W_NCH - 1) / W_NCH;
  const int n0 = nb + ch * per, n1 = (n0 + per < ne) ? n0 + per : ne;
  float num[KP], den[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) num[k] = den[k] = 0.f;
  if (f < Fs) {
#pragma unroll 8
    for (int n = n0; n < n1; ++n) {
      const float pv = P[(size_t)n * Fs + f], av = A1[(size_t)n * Fs + f];
#pragma unroll
      for (int k = 0; k < KP; k += 4) {
        const f32x4 h = *reinterpret_cast<const f32x4*>(Ht + (size_t)n * KP + k);
#pragma unroll
        for (int t = 0; t < 4; ++t) { num[k + t] += pv * h[t]; den[k + t] += av * h[t]; }
      }
    }
    float* dst = part + (((size_t)u * W_NCH + ch) * Fs + f) * 2 * KP;
#pragma unroll
    for (int k = 0; k < KP; k += 4) {
      *reinterpret_cast<f32x4*>(dst + k) = f32x4{num[k], num[k + 1], num[k + 2], num[k + 3]};
      *reinterpret_cast<f32x4*>(dst + KP + k) = f32x4{den[k], den[k + 1], den[k + 2], den[k + 3]};
    }
  }
}

template <int KP>
__global__ __launch_bounds__(640) void w_update_kernel(const float* __restrict__ part, float* __restrict__ W,
                                                       float* __restrict__ normW, int F, int Fs, int K) {
  __shared__ float colred[10][W_KG];
  const int u = blockIdx.x, f = threadIdx.x, k0 = blockIdx.y * W_KG;
  float wn[W_KG];
#pragma unroll
  for (int k = 0; k < W_KG; ++k) wn[k] = 0.f;
  if (f < F) {
    float num[W_KG], den[W_KG];
#pragma unroll
    for (int k = 0; k < W_KG; ++k) num[k] = den[k] = 0.f;
    for (int ch = 0; ch < W_NCH; ++ch) {                 // fixed order: deterministic
      const float* src = part + (((size_t)u * W_NCH + ch) * Fs + f) * 2 * KP;
#pragma unroll
      for (int k = 0; k < W_KG; k += 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(src + k0 + k), b = *reinterpret_cast<const f32x4*>(src + KP + k0 + k);
#pragma unroll
        for (int t = 0; t < 4; ++t) { num[k + t] += a[t]; den[k + t] += b[t]; }
      }
    }
#pragma unroll
    for (int k = 0; k < W_KG; ++k)
      if (k0 + k < K) wn[k] = W[((size_t)u * Fs + f) * KP + k0 + k] * sqrtf(num[k] / den[k]);          // mcem.py:110
  }
  // column L1 norms (mcem.py:129): DPP/permlane wave sum, then across waves in fixed order
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nwv = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int k = 0; k < W_KG; ++k) {
    const float v = sum_rows4(sum_row16(fabsf(wn[k])));
    if (lane == 0) colred[wv][k] = v;
  }
  __syncthreads();
  float nrm[W_KG];
#pragma unroll
  for (int k = 0; k < W_KG; ++k) {
    float s = 0.f;
    for (int ww = 0; ww < nwv; ++ww) s += colred[ww][k];
    nrm[k] = s;
  }
  if (f < Fs) {
#pragma unroll
    for (int k = 0; k < W_KG; ++k)
      W[((size_t)u * Fs + f) * KP + k0 + k] = (k0 + k < K && f < F) ? wn[k] / nrm[k] : 0.f;              // mcem.py:131
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < W_KG; ++k) normW[(size_t)u * KP + k0 + k] = (k0 + k < K) ? nrm[k] : 0.f;         // applied to H (mcem.py:133)
  }
}

// Small batches: wstats_group_kernel (stream.hip) leaves one block of sums per 16-frame GROUP (the groups of utterance u
// follow those of the utterances before it, ceil(N / 16) each).  A 64-frame tile's partial is rebuilt here from its (up to)
// four groups in the order wstats_fused_kernel adds its four wavefronts -- ((g0 + g1) + g2) + g3 -- into the tile layout
// w_update_tiles_kernel reads: the same bits as the tile kernel's.  Block (tile, slot), one thread per bin.
__global__ void w_combine_groups_kernel(const float* __restrict__ part16, const int32_t* __restrict__ tile_g0, const int32_t* __restrict__ tile_cnt,
                                        int F, int Fs, int slots, float* __restrict__ part64) {
  const int T = blockIdx.x, slot = blockIdx.y, f = threadIdx.x;
  if (f >= F) return;
  const int g0 = tile_g0[T], nj = (tile_cnt[T] + 15) / 16;      // the tile's first group and its 1..4 groups (tables of vaenmf_bind_batch)
  const float* src = part16 + ((size_t)g0 * slots + slot) * Fs + f;
  float v = src[0];
  for (int j = 1; j < nj; ++j) v += src[(size_t)j * slots * Fs];
  part64[((size_t)T * slots + slot) * Fs + f] = v;
}

// The same update from the per-tile partial sums of wstats_fused_kernel (stream.hip): part [tile][2 KP][Fs], the tiles of
// utterance u are tile_first[u] .. tile_first[u+1]-1, added in that order; a tile's block is slot-major: [2 k + stat][Fs].
template <int KP>
__global__ __launch_bounds__(640) void w_update_tiles_kernel(const float* __restrict__ part, const int32_t* __restrict__ tile_first,
                                                             float* __restrict__ W, float* __restrict__ normW, int F, int Fs, int K) {
  __shared__ float colred[10][KP];
  const int u = blockIdx.x, f = threadIdx.x;
  float wn[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) wn[k] = 0.f;
  if (f < F) {
    float num[KP], den[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) num[k] = den[k] = 0.f;
    const int t0 = tile_first[u], t1 = tile_first[u + 1];
    for (int t = t0; t < t1; ++t) {                       // fixed order: deterministic
      const float* src = part + (size_t)t * 2 * KP * Fs + f;        // [slot = 2 k + stat][Fs]: coalesced over the bins
#pragma unroll
      for (int k = 0; k < KP; ++k) { num[k] += src[(size_t)(2 * k) * Fs]; den[k] += src[(size_t)(2 * k + 1) * Fs]; }
    }
#pragma unroll
    for (int k = 0; k < KP; ++k)
      if (k < K) wn[k] = W[((size_t)u * Fs + f) * KP + k] * sqrtf(num[k] / den[k]);          // mcem.py:110
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nwv = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    const float v = sum_rows4(sum_row16(fabsf(wn[k])));
    if (lane == 0) colred[wv][k] = v;
  }
  __syncthreads();
  float nrm[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    float s = 0.f;
    for (int ww = 0; ww < nwv; ++ww) s += colred[ww][k];
    nrm[k] = s;
  }
  if (f < Fs) {
#pragma unroll
    for (int k = 0; k < KP; ++k)
      W[((size_t)u * Fs + f) * KP + k] = (k < K && f < F) ? wn[k] / nrm[k] : 0.f;              // mcem.py:131
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < KP; ++k) normW[(size_t)u * KP + k] = (k < K) ? nrm[k] : 0.f;         // applied to H (mcem.py:133)
  }
}

// cost[u][it] = mean_{r,f,n}(log Vx + X2/Vx)  (mcem.py:70) from per-frame sums; block (u, j): iteration it0 + j, whose
// per-frame sums are row j of cost_frames [n_it][stride]
__global__ void cost_reduce_kernel(const double* __restrict__ cost_frames, size_t stride, const int32_t* __restrict__ frame_off,
                                   int R, int F, double* __restrict__ cost, int niter, int it0) {
  __shared__ double red[256];
  const int u = blockIdx.x, j = blockIdx.y;
  const int nb = frame_off[u], ne = frame_off[u + 1];
  const double* cf = cost_frames + (size_t)j * stride;
  double s = 0.0;
  for (int n = nb + threadIdx.x; n < ne; n += blockDim.x) s += cf[n];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int m = 128; m >= 1; m >>= 1) {
    if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
    __syncthreads();
  }
  if (threadIdx.x == 0) cost[(size_t)u * niter + it0 + j] = red[0] / ((double)R * F * (ne - nb));
}

// ----------------------------------------------------------------------------
// Dense layer Y = act(X Wt^T + b), fp32 FMA, 64x64 output tile, K-step 16.
// (encoder / classifier: once per utterance, models.py:101-104, 57-62)
// ----------------------------------------------------------------------------
__device__ __forceinline__ float apply_act(float v, int act) {
  switch (act) {
    case VAENMF_ACT_TANH: return tanhf(v);
    case VAENMF_ACT_RELU: return fmaxf(v, 0.f);
    case VAENMF_ACT_SIGMOID: return 1.0f / (1.0f + expf(-v));
    case VAENMF_ACT_STEP: return v > 0.f ? 1.f : 0.f;
    default: return v;
  }
}
__global__ __launch_bounds__(256) void dense_kernel(const float* __restrict__ X, int M, int in, int ldx,
                                                    const float* __restrict__ Wt, const float* __restrict__ b, int out,
                                                    int act, float* __restrict__ Y, int ldy) {
  __shared__ float xs[16][65], ws[16][65];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int m0 = blockIdx.y * 64, o0 = blockIdx.x * 64;
  float acc[4][4] = {};
  for (int k0 = 0; k0 < in; k0 += 16) {
    for (int e = threadIdx.x; e < 64 * 16; e += 256) {
      const int r = e >> 4, kk = e & 15;
      xs[kk][r] = (m0 + r < M && k0 + kk < in) ? X[(size_t)(m0 + r) * ldx + k0 + kk] : 0.f;
      ws[kk][r] = (o0 + r < out && k0 + kk < in) ? Wt[(size_t)(o0 + r) * in + k0 + kk] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      float xv[4], wv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { xv[i] = xs[kk][ty * 4 + i]; wv[i] = ws[kk][tx * 4 + i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += xv[i] * wv[j];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = m0 + ty * 4 + i, o = o0 + tx * 4 + j;
      if (m < M && o < out) Y[(size_t)m * ldy + o] = apply_act(acc[i][j] + (b ? b[o] : 0.f), act);
    }
}

// |X|^2 = fma(re, re, round(im * im)), spelled out: within one float32 ulp of the exact value, and the power the label
// kernels take (labels.hip).  Left as `re * re + im * im` the compiler emitted a packed multiply and an add: three roundings,
// up to 1.25 ulp (1.14 measured).
__global__ void power_spec_kernel(const float2* __restrict__ X, float* __restrict__ X2, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { const float2 v = X[i]; X2[i] = __fmaf_rn(v.x, v.x, __fmul_rn(v.y, v.y)); }
}

// EM.init_parameters on the device (mcem.py:42-44, :51): W = max(U(0,1), eps) over (F, K), H = max(U(0,1), eps) over
// (K, N), g = 1, padding rows / ranks zero.  Counter-based: the draw of element (utterance, f, k) / (frame inside the
// utterance, k) is splitmix64(utterance seed ^ salt ^ tag ^ index), so an utterance's initialisation does not depend on the
// batch it sits in.  One thread per element of W [U][Fs][Kp] followed by Ht [NT][Kp] and g [NT].
__global__ void nmf_init_kernel(float* __restrict__ W, float* __restrict__ Ht, float* __restrict__ g,
                                const uint64_t* __restrict__ utt_seed, const int32_t* __restrict__ frame_utt,
                                const int32_t* __restrict__ frame_loc, int n_utt, int NT, int F, int Fs, int K, int Kp,
                                uint64_t salt, float eps) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nW = (size_t)n_utt * Fs * Kp, nH = (size_t)NT * Kp;
  auto u01 = [](uint64_t key) {
    uint64_t x = key;
    const uint64_t r = splitmix64(x);
    return (float)(r >> 40) * 5.9604644775390625e-8f;      // 24 bits, [0, 1)
  };
  if (i < nW) {
    const int k = (int)(i % Kp), f = (int)((i / Kp) % Fs), u = (int)(i / ((size_t)Kp * Fs));
    float v = 0.f;
    if (f < F && k < K) v = fmaxf(u01(utt_seed[u] ^ salt ^ (0x57ull << 56) ^ (uint64_t)(f * K + k)), eps);
    W[i] = v;
  } else if (i < nW + nH) {
    const size_t j = i - nW;
    const int k = (int)(j % Kp), n = (int)(j / Kp);
    float v = 0.f;
    if (k < K) v = fmaxf(u01(utt_seed[frame_utt[n]] ^ salt ^ (0x48ull << 56) ^ ((uint64_t)frame_loc[n] * (uint64_t)K + (uint64_t)k)), eps);
    Ht[j] = v;
  } else if (i < nW + nH + (size_t)NT) {
    g[i - nW - nH] = 1.f;
  }
}

// Gram matrix of (s_hat, s, n) per utterance in float64 (python/metrics.py:12-60)
__global__ __launch_bounds__(256) void gram3_kernel(const float* __restrict__ sh, const float* __restrict__ s,
                                                    const float* __restrict__ nz, const int64_t* __restrict__ samp_off,
                                                    double* __restrict__ out) {
  __shared__ double red[6][256];
  const int u = blockIdx.x;
  const int64_t b = samp_off[u], e = samp_off[u + 1];
  double a[6] = {0, 0, 0, 0, 0, 0};
  for (int64_t i = b + threadIdx.x; i < e; i += blockDim.x) {
    const double x = sh[i], y = s[i], z = nz[i];
    a[0] += x * x; a[1] += x * y; a[2] += x * z; a[3] += y * y; a[4] += y * z; a[5] += z * z;
  }
  for (int j = 0; j < 6; ++j) red[j][threadIdx.x] = a[j];
  __syncthreads();
  for (int m = 128; m >= 1; m >>= 1) {
    if ((int)threadIdx.x < m)
      for (int j = 0; j < 6; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + m];
    __syncthreads();
  }
  if (threadIdx.x < 6) out[(size_t)u * 6 + threadIdx.x] = red[threadIdx.x][0];
}


// HBM read probe (bench.py's measured ceiling for the streaming M-step kernels): every lane keeps UNR 16-byte loads in
// flight, a workgroup sweeps contiguous 4 KB pieces in a grid-stride loop, the grid is the resident set (8 workgroups of
// 256 threads per CU = 8 wavefronts per SIMD).  The loaded words are folded into one value per lane that is stored only
// if it equals a sentinel the data never produces, so nothing is written and nothing is optimised away.
template <int UNR>
__global__ __launch_bounds__(256) void hbm_read_probe_kernel(const u32x4p* __restrict__ buf, size_t n16, unsigned* sink) {
  const size_t stride = (size_t)gridDim.x * 256 * UNR;
  unsigned acc = 0;
  size_t i = (size_t)blockIdx.x * 256 * UNR + threadIdx.x;
  for (; i + (size_t)(UNR - 1) * 256 < n16; i += stride) {
    u32x4p v[UNR];
#pragma unroll
    for (int k = 0; k < UNR; ++k) v[k] = __builtin_nontemporal_load(buf + i + (size_t)k * 256);
#pragma unroll
    for (int k = 0; k < UNR; ++k) acc ^= v[k][0] ^ v[k][1] ^ v[k][2] ^ v[k][3];
  }
  for (; i < n16; i += 256) { const u32x4p v = buf[i]; acc ^= v[0] ^ v[1] ^ v[2] ^ v[3]; }
  if (acc == 0x9E3779B9u) sink[0] = acc;
}

// Wavefront-sum probe (tests): one wavefront per set of 4 x 64 floats.  Every lane writes what it holds of the four totals
// taken one at a time (sum_rows4 of sum_row16, as wave_sum of stream.hip), of the four through one shared cross-row stage
// (sum_rows4_x4: row j = total j) and of two pairs (sum_rows4_x2: rows 0 and 2 = the first, rows 1 and 3 = the second).
__global__ __launch_bounds__(64) void wave_sum_probe_kernel(const float* __restrict__ x, float* one, float* x4, float* x2) {
  const size_t set = blockIdx.x;
  const int lane = threadIdx.x;
  float v[4], r[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    v[q] = x[(set * 4 + q) * 64 + lane];
    r[q] = sum_row16(v[q]);
    one[(set * 4 + q) * 64 + lane] = sum_rows4(r[q]);
  }
  x4[set * 64 + lane] = sum_rows4_x4(r[0], r[1], r[2], r[3]);
  x2[(set * 2 + 0) * 64 + lane] = sum_rows4_x2(r[0], r[1]);
  x2[(set * 2 + 1) * 64 + lane] = sum_rows4_x2(r[2], r[3]);
}

}  // namespace

int vn_launch_w_update(const vaenmf_plan* p, float* W, const float* Ht, hipStream_t st) {
  const int threads = ((p->Fs + 63) / 64) * 64;        // one thread per bin (Fs <= 640)
#define VN_WU(KP)                                                                                               \
  do {                                                                                                          \
    hipLaunchKernelGGL((w_partial_kernel<KP>), dim3(W_NCH, p->n_utt), dim3(threads), 0, st, p->A1, p->P, Ht, \
                       p->wpart, p->d_frame_off, p->Fs);                                                        \
    hipLaunchKernelGGL((w_update_kernel<KP>), dim3(p->n_utt, KP / W_KG), dim3(threads), 0, st, p->wpart, W, p->normW, \
                       p->cfg.F, p->Fs, p->cfg.K);                                                               \
  } while (0)
  switch (p->Kp) { case 8: VN_WU(8); break; case 16: VN_WU(16); break; default: VN_WU(32); break; }
#undef VN_WU
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

int vn_launch_w_update_tiles(const vaenmf_plan* p, float* W, hipStream_t st, bool groups) {
  const int threads = ((p->Fs + 63) / 64) * 64;
  if (groups) {                                           // group sums -> tile partials (small batches)
    VN_REQUIRE(p->wpart16, "group partials: rank <= 8 only");
    hipLaunchKernelGGL(w_combine_groups_kernel, dim3(p->n_t64, 2 * p->Kp), dim3(threads), 0, st, p->wpart16, p->d_t64_g0, p->d_t64_cnt,
                       p->cfg.F, p->Fs, 2 * p->Kp, p->wpart64);
  }
  switch (p->Kp) {
    case 8: hipLaunchKernelGGL((w_update_tiles_kernel<8>), dim3(p->n_utt), dim3(threads), 0, st, p->wpart64, p->d_t64_first, W, p->normW, p->cfg.F, p->Fs, p->cfg.K); break;
    case 16: hipLaunchKernelGGL((w_update_tiles_kernel<16>), dim3(p->n_utt), dim3(threads), 0, st, p->wpart64, p->d_t64_first, W, p->normW, p->cfg.F, p->Fs, p->cfg.K); break;
    default: hipLaunchKernelGGL((w_update_tiles_kernel<32>), dim3(p->n_utt), dim3(threads), 0, st, p->wpart64, p->d_t64_first, W, p->normW, p->cfg.F, p->Fs, p->cfg.K); break;
  }
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

// n_it consecutive iterations it0 .. it0 + n_it - 1 in one launch (cost_frames: n_it rows of `stride` doubles)
int vn_launch_cost_reduce(const vaenmf_plan* p, const double* cost_frames, size_t stride, int n_it, int R, double* cost, int niter, int it0, hipStream_t st) {
  hipLaunchKernelGGL(cost_reduce_kernel, dim3(p->n_utt, n_it), dim3(256), 0, st, cost_frames, stride, p->d_frame_off, R, p->cfg.F, cost, niter, it0);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int vaenmf_dense(const float* X, int32_t M, int32_t in, int32_t ldx, const float* Wt, const float* b,
                            int32_t out, int32_t act, float* Y, int32_t ldy, void* stream) {
  VN_REQUIRE(X && Wt && Y && M > 0 && in > 0 && out > 0, "vaenmf_dense: bad arguments");
  hipLaunchKernelGGL(dense_kernel, dim3((out + 63) / 64, (M + 63) / 64), dim3(256), 0, (hipStream_t)stream, X, M, in, ldx,
                     Wt, b, out, act, Y, ldy);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int vaenmf_power_spec(const float* X, float* X2, int64_t n, void* stream) {
  VN_REQUIRE(X && X2 && n > 0, "vaenmf_power_spec: bad arguments");
  hipLaunchKernelGGL(power_spec_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float2*>(X), X2, n);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int vaenmf_init_nmf(vaenmf_plan* p, float* W, float* Ht, float* g, uint64_t salt, float eps, void* stream) {
  VN_REQUIRE(p && W && Ht && g && p->NT > 0, "vaenmf_init_nmf: null argument or no batch bound");
  const size_t n = (size_t)p->n_utt * p->Fs * p->Kp + (size_t)p->NT * p->Kp + (size_t)p->NT;
  hipLaunchKernelGGL(nmf_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, W, Ht, g, p->d_utt_seed,
                     p->d_frame_utt, p->d_frame_loc, p->n_utt, p->NT, p->cfg.F, p->Fs, p->cfg.K, p->Kp, salt, eps);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int vaenmf_gram3_batch(const float* s_hat, const float* s, const float* n, int32_t n_utt,
                                  const int64_t* sample_offsets, double* out, void* stream) {
  VN_REQUIRE(s_hat && s && n && out && n_utt > 0, "vaenmf_gram3_batch: bad arguments");
  hipLaunchKernelGGL(gram3_kernel, dim3(n_utt), dim3(256), 0, (hipStream_t)stream, s_hat, s, n, sample_offsets, out);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

// Measurement aid of bench.py (not on the hot path): the rate at which this GPU delivers a plain streaming read of `bytes`
// bytes of `buf` (DEV, 16-byte aligned) to a hand-written kernel -- 16 bytes per lane, 8 wavefronts per SIMD, 4 loads in
// flight per lane.  `reps` timed sweeps after one untimed sweep, HIP events on `stream`; synchronises.  sink DEV: 4 bytes.
extern "C" int vaenmf_hbm_read_probe(const void* buf, int64_t bytes, int32_t reps, void* sink, double* gbps_out, void* stream) {
  VN_REQUIRE(buf && sink && gbps_out && bytes >= (1 << 20) && reps > 0, "vaenmf_hbm_read_probe: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  int dev = 0, cus = 256;
  VN_CHECK_HIP(hipGetDevice(&dev));
  VN_CHECK_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  hipEvent_t e0, e1;
  VN_CHECK_HIP(hipEventCreate(&e0));
  VN_CHECK_HIP(hipEventCreate(&e1));
  const size_t n16 = (size_t)bytes / 16;
  auto sweep = [&]() { hipLaunchKernelGGL((hbm_read_probe_kernel<4>), dim3(cus * 8), dim3(256), 0, st, reinterpret_cast<const u32x4p*>(buf), n16, reinterpret_cast<unsigned*>(sink)); };
  sweep();
  (void)hipEventRecord(e0, st);
  for (int r = 0; r < reps; ++r) sweep();
  (void)hipEventRecord(e1, st);
  hipError_t e = hipEventSynchronize(e1);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  VN_CHECK_HIP(e);
  VN_CHECK_HIP(hipGetLastError());
  *gbps_out = (double)(n16 * 16) * reps / ((double)ms * 1e-3) / 1e9;
  return 0;
}

// Test aid (not on the hot path): the wavefront sums of common.h on n sets of 4 x 64 floats, x DEV [n][4][64].  Written per
// lane: one DEV [n][4][64] each value summed on its own (sum_rows4 of sum_row16), x4 DEV [n][64] the four through
// sum_rows4_x4 (lanes 16 j .. 16 j + 15 hold total j), x2 DEV [n][2][64] the pairs (0, 1) and (2, 3) through sum_rows4_x2
// (lanes 0-15 and 32-47 hold the pair's first total, lanes 16-31 and 48-63 its second).
extern "C" int vaenmf_wave_sum_probe(const float* x, int32_t n, float* one, float* x4, float* x2, void* stream) {
  VN_REQUIRE(x && one && x4 && x2 && n > 0, "vaenmf_wave_sum_probe: bad arguments");
  hipLaunchKernelGGL(wave_sum_probe_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, x, one, x4, x2);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}
