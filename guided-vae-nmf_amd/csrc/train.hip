// The training step of the reference's three scripts (scripts/training_M1.py, training_M2.py, training_classifier.py) on
// the device: dense layers forward and backward on the fp32-input matrix instruction, the ELBO and BCE heads
// (python/models/utils.py: elbo, binary_cross_entropy), batch assembly, torch.optim.Adam's update and the trainer that
// strings them together launch after launch on one stream.  include/vaenmf.h states the contracts.
//
// Everything is fp32 with fp32 accumulation; loss sums are double.  What a step computes does not depend on the run:
//   - a dense product is v_mfma_f32_16x16x4_f32 over k in ascending order, which is bit for bit the chain
//     fmaf(a_k, b_k, acc); an output element is four such chains -- chain j takes the k with (k / 4) % 4 == j -- and the
//     bias, added with two-sums whose rounding errors go back in once (sum_chains); k past the reduction length enters as the product 0 * 0 and leaves its chain as it was.  The
//     reduction of dW / db is the batch and one workgroup walks all of it: no split-K across workgroups, no atomics.
//   - a row's loss terms are summed by its workgroup (lanes by the xor butterfly, waves in wave order) and the rows by one
//     workgroup in the same manner.
//   - operands are read one float at its natural alignment, never past the M x K / K x N extent: what lies between a row's
//     last column and its leading dimension is neither read nor written.
#include <math.h>
#include <new>
#include <string.h>
#include <vector>
#include "common.h"

namespace {

constexpr int TM = 32, TN = 64, TK = 64;     // output tile of a workgroup (4 waves: 2 x 2 of 16 x 32), k per LDS stage (24 KiB: a stage's
                                             // loads are all in flight together; the layers are latency-bound, 8 .. 36 workgroups)
constexpr int GEMM_THREADS = 256;
constexpr int ROW_THREADS = 256;
enum { EPI_FWD = 0, EPI_DX = 1, EPI_DW = 2 };

struct GemmArgs {
  const float *A, *B;         // A(m, k) = A[m sam + k sak], B(k, n) = B[k sbk + n sbn]
  int64_t sam, sak, sbk, sbn;
  int M, N, K;
  float* C; int ldc;          // C[m ldc + n]
  const float* bias; int act; // EPI_FWD: C = act(acc + bias[n])
  const float* Yp; int ldp;   // EPI_DX: C = acc * act'(Yp[m ldp + n]) from the saved activated output
  float* db;                  // EPI_DW: db[m] = sum_k A(m, k) (the workgroups of the first column tile), or null
};

__device__ __forceinline__ float act_fwd(float v, int act) {
  switch (act) {
    case VAENMF_ACT_TANH: return tanhf(v);
    case VAENMF_ACT_RELU: return v > 0.0f ? v : 0.0f;
    case VAENMF_ACT_SIGMOID: return 1.0f / (1.0f + expf(-v));
    case VAENMF_ACT_EXP: return expf(v);
    default: return v;
  }
}
__device__ __forceinline__ float act_deriv(float y, int act) {
  switch (act) {
    case VAENMF_ACT_TANH: return 1.0f - y * y;
    case VAENMF_ACT_RELU: return y > 0.0f ? 1.0f : 0.0f;
    case VAENMF_ACT_SIGMOID: return y * (1.0f - y);
    case VAENMF_ACT_EXP: return y;
    default: return 1.0f;
  }
}

// a + b = s + e exactly (Knuth's two-sum, fp32 throughout)
__device__ __forceinline__ void two_sum(float a, float b, float& s, float& e) {
  s = a + b;
  const float bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}
// the four chains of an output element and its bias in one rounding instead of four: the sums' rounding errors are kept
// and added back once (the additions were three quarters of the error variance of a 16-term product)
__device__ __forceinline__ float sum_chains(float c0, float c1, float c2, float c3, float b) {
  float s01, e01, s23, e23, s, e, t, et;
  two_sum(c0, c1, s01, e01);
  two_sum(c2, c3, s23, e23);
  two_sum(s01, s23, s, e);
  two_sum(s, b, t, et);
  return t + (((e01 + e23) + e) + et);
}

// AK / BK: k is the unit-stride index of A / B (decides which index runs along the lanes of a staging load)
template <bool AK, bool BK, int EPI>
__global__ __launch_bounds__(GEMM_THREADS) void train_gemm_kernel(GemmArgs g) {
  __shared__ float As[TK][TM + 1], Bs[TK][TN + 1];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
  const int wm = (wave & 1) * 16, wn = (wave >> 1) * 32;
  const int lr = lane & 15, lk = lane >> 4;
  const bool with_db = EPI == EPI_DW && g.db != nullptr && blockIdx.x == 0 && wn == 0;
  // four chains per output element: MFMA step s of a k stage feeds accumulator s % 4 (independent accumulators keep
  // the matrix pipe issuing, and a chain a quarter as long rounds less), summed at the end by sum_chains
  const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
  f32x4 acc0[4] = {zero4, zero4, zero4, zero4}, acc1[4] = {zero4, zero4, zero4, zero4}, accb[4] = {zero4, zero4, zero4, zero4};
  for (int k0 = 0; k0 < g.K; k0 += TK) {
    for (int e = tid; e < TM * TK; e += GEMM_THREADS) {
      const int k = AK ? e % TK : e / TM, m = AK ? e / TK : e % TM;
      const int gm = m0 + m, gk = k0 + k;
      As[k][m] = (gm < g.M && gk < g.K) ? g.A[gm * g.sam + gk * g.sak] : 0.0f;
    }
    for (int e = tid; e < TN * TK; e += GEMM_THREADS) {
      const int k = BK ? e % TK : e / TN, n = BK ? e / TK : e % TN;
      const int gn = n0 + n, gk = k0 + k;
      Bs[k][n] = (gn < g.N && gk < g.K) ? g.B[gk * g.sbk + gn * g.sbn] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < TK / 4; ++s) {
      const int j = s & 3;
      const float a = As[4 * s + lk][wm + lr];
      acc0[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[4 * s + lk][wn + lr], acc0[j], 0, 0, 0);
      acc1[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[4 * s + lk][wn + 16 + lr], acc1[j], 0, 0, 0);
      if (with_db) accb[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, 1.0f, accb[j], 0, 0, 0);   // every column: the row sums of A
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = m0 + wm + lk * 4 + r;
    if (m >= g.M) continue;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int n = n0 + wn + 16 * t + lr;
      if (n >= g.N) continue;
      const float bias = (EPI == EPI_FWD && g.bias) ? g.bias[n] : 0.0f;
      float v = t ? sum_chains(acc1[0][r], acc1[1][r], acc1[2][r], acc1[3][r], bias) : sum_chains(acc0[0][r], acc0[1][r], acc0[2][r], acc0[3][r], bias);
      if (EPI == EPI_FWD) v = act_fwd(v, g.act);
      if (EPI == EPI_DX && g.Yp) v *= act_deriv(g.Yp[(int64_t)m * g.ldp + n], g.act);
      g.C[(int64_t)m * g.ldc + n] = v;
    }
    if (with_db && lr == 0) g.db[m] = sum_chains(accb[0][r], accb[1][r], accb[2][r], accb[3][r], 0.0f);
  }
}

int launch_gemm(int epi, const GemmArgs& g, hipStream_t st) {
  const dim3 grid((unsigned)((g.N + TN - 1) / TN), (unsigned)((g.M + TM - 1) / TM)), block(GEMM_THREADS);
  if (epi == EPI_FWD) hipLaunchKernelGGL((train_gemm_kernel<true, true, EPI_FWD>), grid, block, 0, st, g);
  else if (epi == EPI_DX) hipLaunchKernelGGL((train_gemm_kernel<true, false, EPI_DX>), grid, block, 0, st, g);
  else hipLaunchKernelGGL((train_gemm_kernel<false, false, EPI_DW>), grid, block, 0, st, g);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

// Y[M][out] = act(X[M][in] W[out][in]^T + b)
int gemm_fwd(const float* X, int M, int in, int ldx, const float* W, int ldw, const float* b, int out, int act, float* Y, int ldy,
             hipStream_t st) {
  GemmArgs g = {};
  g.A = X; g.sam = ldx; g.sak = 1; g.B = W; g.sbk = 1; g.sbn = ldw;
  g.M = M; g.N = out; g.K = in; g.C = Y; g.ldc = ldy; g.bias = b; g.act = act;
  return launch_gemm(EPI_FWD, g, st);
}
// dX[M][in] = (dZ[M][out] W[out][in]) * act'(Yprev[M][in])
int gemm_dx(const float* dZ, int M, int out, int ldz, const float* W, int ldw, int in, const float* Yp, int ldp, int act, float* dX,
            int lddx, hipStream_t st) {
  GemmArgs g = {};
  g.A = dZ; g.sam = ldz; g.sak = 1; g.B = W; g.sbk = ldw; g.sbn = 1;
  g.M = M; g.N = in; g.K = out; g.C = dX; g.ldc = lddx; g.Yp = Yp; g.ldp = ldp; g.act = act;
  return launch_gemm(EPI_DX, g, st);
}
// dW[out][in] = dZ[M][out]^T X[M][in], db[out] = column sums of dZ
int gemm_dw(const float* dZ, int M, int out, int ldz, const float* X, int in, int ldx, float* dW, int lddw, float* db, hipStream_t st) {
  GemmArgs g = {};
  g.A = dZ; g.sam = 1; g.sak = ldz; g.B = X; g.sbk = ldx; g.sbn = 1;
  g.M = out; g.N = in; g.K = M; g.C = dW; g.ldc = lddw; g.db = db;
  return launch_gemm(EPI_DW, g, st);
}

// ---- sums in a fixed order ----
template <int THREADS>
__device__ __forceinline__ double tr_block_sum(double v, double* red) {     // every thread gets the sum
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
  if (THREADS == 64) return v;
  __syncthreads();                        // red may still be read from the previous sum
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = red[0];
#pragma unroll
  for (int i = 1; i < THREADS / 64; ++i) r += red[i];
  return r;
}

// ---- ELBO head at the output: one workgroup per row ----
__global__ __launch_bounds__(ROW_THREADS) void elbo_out_kernel(const float* __restrict__ X, int ldx, const float* __restrict__ A, int lda,
                                                               int F, double eps, float inv_b, float* __restrict__ dA, int ldd,
                                                               double* __restrict__ row_recon) {
  __shared__ double red[ROW_THREADS / 64];
  const int b = blockIdx.x;
  double s = 0.0;
  for (int f = threadIdx.x; f < F; f += ROW_THREADS) {
    const float x = X[(int64_t)b * ldx + f], a = A[(int64_t)b * lda + f];
    const float r = expf(a);
    s += (double)x / (double)r - log((double)x + eps) + (double)a - 1.0;
    if (dA) dA[(int64_t)b * ldd + f] = (1.0f - x / r) * inv_b;
  }
  s = tr_block_sum<ROW_THREADS>(s, red);
  if (threadIdx.x == 0) row_recon[b] = s;
}

// ---- ELBO head at the latent: one wavefront per row; ML holds mu in columns 0 .. z-1 and logvar in z .. 2z-1 ----
__global__ __launch_bounds__(64) void latent_fwd_kernel(const float* __restrict__ ML, int ldm, const float* __restrict__ eps, int z,
                                                        float* __restrict__ Z, int ldz) {
  const int b = blockIdx.x;
  for (int j = threadIdx.x; j < z; j += 64) {
    const float mu = ML[(int64_t)b * ldm + j], lv = ML[(int64_t)b * ldm + z + j];
    Z[(int64_t)b * ldz + j] = fmaf(expf(0.5f * lv), eps[(int64_t)b * z + j], mu);
  }
}

__global__ __launch_bounds__(64) void latent_bwd_kernel(const float* __restrict__ ML, int ldm, const float* __restrict__ eps,
                                                        const float* __restrict__ dZ, int lddz, int z, float inv_b,
                                                        float* __restrict__ dML, int lddm, double* __restrict__ row_kl) {
  const int b = blockIdx.x;
  double s = 0.0;
  for (int j = threadIdx.x; j < z; j += 64) {
    const float mu = ML[(int64_t)b * ldm + j], lv = ML[(int64_t)b * ldm + z + j];
    s += (double)lv - (double)mu * (double)mu - exp((double)lv);
    if (dML) {
      const float dz = dZ[(int64_t)b * lddz + j];
      dML[(int64_t)b * lddm + j] = mu * inv_b + dz;
      dML[(int64_t)b * lddm + z + j] = 0.5f * (expf(lv) - 1.0f) * inv_b + 0.5f * dz * expf(0.5f * lv) * eps[(int64_t)b * z + j];
    }
  }
  s = tr_block_sum<64>(s, nullptr);
  if (threadIdx.x == 0) row_kl[b] = -0.5 * s;
}

// ---- BCE head: one workgroup per row; the terms are evaluated in double from the float pre-activation ----
__global__ __launch_bounds__(ROW_THREADS) void bce_head_kernel(const float* __restrict__ A, int lda, const float* __restrict__ Y, int ldy,
                                                               int D, double eps, double inv_b, float* __restrict__ dA, int ldd,
                                                               double* __restrict__ row_loss, int32_t* __restrict__ row_cnt) {
  __shared__ double red[ROW_THREADS / 64];
  const int b = blockIdx.x;
  double s = 0.0, tp = 0.0, tn = 0.0, fp = 0.0, fn = 0.0;
  for (int j = threadIdx.x; j < D; j += ROW_THREADS) {
    const double a = (double)A[(int64_t)b * lda + j], y = (double)Y[(int64_t)b * ldy + j];
    // yh = sigmoid(a) and q = 1 - yh = sigmoid(-a), each from the exponential that does not overflow
    const double e = exp(-fabs(a));
    const double big = 1.0 / (1.0 + e), small = e / (1.0 + e);
    const double yh = a >= 0.0 ? big : small, q = a >= 0.0 ? small : big;
    s -= y * log(yh + eps) + (1.0 - y) * log(q + eps);
    if (dA) dA[(int64_t)b * ldd + j] = (float)(-(y / (yh + eps) - (1.0 - y) / (q + eps)) * yh * q * inv_b);
    const bool pred = yh > 0.5, lab = y > 0.5;
    tp += (pred && lab) ? 1.0 : 0.0; tn += (!pred && !lab) ? 1.0 : 0.0;
    fp += (pred && !lab) ? 1.0 : 0.0; fn += (!pred && lab) ? 1.0 : 0.0;
  }
  s = tr_block_sum<ROW_THREADS>(s, red);
  tp = tr_block_sum<ROW_THREADS>(tp, red); tn = tr_block_sum<ROW_THREADS>(tn, red);
  fp = tr_block_sum<ROW_THREADS>(fp, red); fn = tr_block_sum<ROW_THREADS>(fn, red);
  if (threadIdx.x == 0) {
    row_loss[b] = s;
    int32_t* c = row_cnt + (int64_t)b * 4;
    c[0] = (int32_t)tp; c[1] = (int32_t)tn; c[2] = (int32_t)fp; c[3] = (int32_t)fn;      // counts below 2^31: exact in double
  }
}

// ---- the rows' sums to the step's result: one workgroup ----
// out: double loss, recon, KL, 0 then int64 tp, tn, fp, fn.  row_b / row_cnt may be null.
__global__ __launch_bounds__(ROW_THREADS) void loss_reduce_kernel(const double* __restrict__ row_a, const double* __restrict__ row_b,
                                                                  const int32_t* __restrict__ row_cnt, int B, double* __restrict__ out) {
  __shared__ double red[ROW_THREADS / 64];
  double sa = 0.0, sb = 0.0, c[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < B; b += ROW_THREADS) {
    sa += row_a[b];
    if (row_b) sb += row_b[b];
    if (row_cnt)
      for (int i = 0; i < 4; ++i) c[i] += (double)row_cnt[(int64_t)b * 4 + i];
  }
  sa = tr_block_sum<ROW_THREADS>(sa, red);
  sb = tr_block_sum<ROW_THREADS>(sb, red);
  for (int i = 0; i < 4; ++i) c[i] = tr_block_sum<ROW_THREADS>(c[i], red);
  if (threadIdx.x == 0) {
    const double ma = sa / (double)B, mb = sb / (double)B;
    out[0] = ma + mb; out[1] = ma; out[2] = mb; out[3] = 0.0;
    int64_t* oc = reinterpret_cast<int64_t*>(out + 4);
    for (int i = 0; i < 4; ++i) oc[i] = (int64_t)c[i];
  }
}

// ---- batch assembly: dst[b][col0 + c] = src[idx[b]][c], c < ncol, normalised when mean / std are given ----
__global__ __launch_bounds__(ROW_THREADS) void train_gather_kernel(const float* __restrict__ src, int64_t lds, int64_t NT,
                                                                   const int32_t* __restrict__ idx, int ncol, const float* __restrict__ mean,
                                                                   const float* __restrict__ std, float eps, float* __restrict__ dst,
                                                                   int ldd, int col0) {
  const int b = blockIdx.x;
  const int64_t i = idx[b];
  const bool ok = i >= 0 && i < NT;             // a row outside the matrix is not read: NaN marks the mistake
  for (int c = threadIdx.x; c < ncol; c += ROW_THREADS) {
    float v = ok ? src[i * lds + c] : __builtin_nanf("");
    if (mean) v = (v - mean[c]) / (std[c] + eps);
    dst[(int64_t)b * ldd + col0 + c] = v;
  }
}

// ---- torch.optim.Adam (single-tensor path): lerp_, mul_().addcmul_(), sqrt / bias_correction2_sqrt + eps, addcdiv_ ----
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t n, float w1, float beta2, float w2, float neg_step,
                                                   float bc2_sqrt, float eps) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float gi = g[i];
  const float mi = m[i] + w1 * (gi - m[i]);
  const float vi = v[i] * beta2 + (w2 * gi) * gi;
  m[i] = mi; v[i] = vi;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  p[i] = p[i] + (neg_step * mi) / denom;
}

// ---- reparameterisation draws: z / 4 streams of four normals per row, keyed by (seed, step, row) ----
__global__ __launch_bounds__(256) void train_eps_kernel(uint64_t key, uint32_t step, int B, int z, float* __restrict__ eps) {
  const int q4 = z / 4;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * q4) return;
  const int b = i / q4, q = i % q4;
  Xs128 st = xs_seed(key ^ ((uint64_t)(q >> 8) << 40), (uint32_t)b, (uint32_t)(q & 255), step);
  const f32x4 nrm = normal4(st);
#pragma unroll
  for (int t = 0; t < 4; ++t) eps[(int64_t)b * z + 4 * q + t] = nrm[t];
}

int launch_eps(uint64_t seed, uint32_t step, int B, int z, float* eps, hipStream_t st) {
  uint64_t x = seed;
  const uint64_t key = splitmix64(x);            // neighbouring seeds share no stream
  hipLaunchKernelGGL(train_eps_kernel, dim3((unsigned)((B * (z / 4) + 255) / 256)), dim3(256), 0, st, key, step, B, z, eps);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

struct Layer {
  int in, out, act;
  size_t w, b;           // offsets into the parameter arena (floats): W [out][in], b [out]
};
struct Tensor {          // a tensor of the state_dict, in its order
  size_t off; int rows, cols;
};

}  // namespace

struct vaenmf_trainer {
  vaenmf_trainer_config cfg;
  std::vector<Layer> enc, dec;    // M1 / M2: encoder (hidden .., [mu | logvar]) and decoder (hidden .., reconstruction); classifier: enc only
  std::vector<Tensor> tensors;
  size_t n_params = 0;
  float* arena = nullptr;         // [4][n_params]: parameters, gradients, Adam m, Adam v
  float* act = nullptr;           // activations and their gradients
  double* rows = nullptr;         // [2][max_batch] per-row loss terms
  int32_t* row_cnt = nullptr;     // [max_batch][4]
  float* eps = nullptr;           // [max_batch][z]: the draws of a DEVICE-mode step
  const float *mean = nullptr, *std = nullptr;
  float norm_eps = 0.0f;
  int in0 = 0, d0 = 0;            // width of the encoder's / the decoder's input
  std::vector<float*> ea, eg, da, dg;   // enc / dec: output of layer i and its gradient ([max_batch][out])
  float *x_in = nullptr, *d_in = nullptr, *d_in_g = nullptr, *ybatch = nullptr;
  int64_t step = 0;
  float* P() const { return arena; }
  float* G() const { return arena + n_params; }
  float* Mo() const { return arena + 2 * n_params; }
  float* Vo() const { return arena + 3 * n_params; }
};

namespace {

constexpr int TR_MAX_DIM = 4096, TR_MAX_BATCH = 65536;

void add_layer(vaenmf_trainer* t, std::vector<Layer>& net, int in, int out, int act, bool split) {
  Layer l;
  l.in = in; l.out = out; l.act = act;
  l.w = t->n_params; t->n_params += (size_t)in * out;
  l.b = t->n_params; t->n_params += (size_t)out;
  net.push_back(l);
  if (split) {             // [mu | logvar]: four tensors of the state_dict, two halves of one layer
    const int z = out / 2;
    t->tensors.push_back({l.w, z, in}); t->tensors.push_back({l.b, z, 0});
    t->tensors.push_back({l.w + (size_t)z * in, z, in}); t->tensors.push_back({l.b + z, z, 0});
  } else {
    t->tensors.push_back({l.w, out, in}); t->tensors.push_back({l.b, out, 0});
  }
}

int forward_net(const vaenmf_trainer* t, const std::vector<Layer>& net, const std::vector<float*>& outs, const float* in, int ldin, int B,
                hipStream_t st) {
  for (size_t i = 0; i < net.size(); ++i) {
    const Layer& l = net[i];
    const float* x = i ? outs[i - 1] : in;
    const int ldx = i ? net[i - 1].out : ldin;
    if (int rc = gemm_fwd(x, B, l.in, ldx, t->P() + l.w, l.in, t->P() + l.b, l.out, l.act, outs[i], l.out, st)) return rc;
  }
  return 0;
}

// grads[last] holds the gradient at the last layer's pre-activation; din_g (or null): gradient at the first n_din columns of the input
int backward_net(const vaenmf_trainer* t, const std::vector<Layer>& net, const std::vector<float*>& outs, const std::vector<float*>& grads,
                 const float* in, int ldin, float* din_g, int n_din, int B, hipStream_t st) {
  for (size_t i = net.size(); i-- > 0;) {
    const Layer& l = net[i];
    const float* x = i ? outs[i - 1] : in;
    const int ldx = i ? net[i - 1].out : ldin;
    if (int rc = gemm_dw(grads[i], B, l.out, l.out, x, l.in, ldx, t->G() + l.w, l.in, t->G() + l.b, st)) return rc;
    if (i) {
      if (int rc = gemm_dx(grads[i], B, l.out, l.out, t->P() + l.w, l.in, l.in, outs[i - 1], net[i - 1].out, net[i - 1].act, grads[i - 1],
                           net[i - 1].out, st))
        return rc;
    } else if (din_g) {
      if (int rc = gemm_dx(grads[i], B, l.out, l.out, t->P() + l.w, l.in, n_din, nullptr, 0, VAENMF_ACT_NONE, din_g, n_din, st)) return rc;
    }
  }
  return 0;
}

int check_step_args(const char* fn, const vaenmf_trainer* t, const float* X, int32_t ldx, const float* Y, int32_t ldy, int64_t NT,
                    const int32_t* idx, int32_t B, const double* losses) {
  VN_REQUIRE(t != nullptr, "%s: null trainer", fn);
  const vaenmf_trainer_config& c = t->cfg;
  VN_REQUIRE(B >= 1 && B <= c.max_batch, "%s: B=%d outside [1, max_batch=%d]", fn, B, c.max_batch);
  VN_REQUIRE(NT >= 1 && NT <= INT32_MAX, "%s: NT=%lld outside [1, 2^31)", fn, (long long)NT);
  VN_REQUIRE(X && idx && losses, "%s: null X / idx / losses", fn);
  VN_REQUIRE(ldx >= c.x_dim, "%s: ldx=%d < x_dim=%d", fn, ldx, c.x_dim);
  VN_REQUIRE(((uintptr_t)losses & 7) == 0, "%s: losses must be aligned to 8 bytes", fn);
  if (c.kind != VAENMF_TRAIN_M1) {
    VN_REQUIRE(Y != nullptr, "%s: this model needs labels Y", fn);
    VN_REQUIRE(ldy >= c.y_dim, "%s: ldy=%d < y_dim=%d", fn, ldy, c.y_dim);
  }
  return 0;
}

// forward (and, with train, backward and Adam) of one batch
int run_step(vaenmf_trainer* t, bool train, const float* X, int32_t ldx, const float* Y, int32_t ldy, int64_t NT, const int32_t* idx, int32_t B,
             const float* eps, uint64_t seed, double* losses, hipStream_t st) {
  const vaenmf_trainer_config& c = t->cfg;
  const float inv_b = 1.0f / (float)B;
  const dim3 rows((unsigned)B), rt(ROW_THREADS);
  const bool cls = c.kind == VAENMF_TRAIN_CLASSIFIER;
  hipLaunchKernelGGL(train_gather_kernel, rows, rt, 0, st, X, (int64_t)ldx, NT, idx, c.x_dim, cls ? t->mean : nullptr, cls ? t->std : nullptr,
                     t->norm_eps, t->x_in, t->in0, 0);
  VN_CHECK_HIP(hipGetLastError());
  if (cls) {
    hipLaunchKernelGGL(train_gather_kernel, rows, rt, 0, st, Y, (int64_t)ldy, NT, idx, c.y_dim, nullptr, nullptr, 0.0f, t->ybatch, c.y_dim, 0);
    VN_CHECK_HIP(hipGetLastError());
    if (int rc = forward_net(t, t->enc, t->ea, t->x_in, t->in0, B, st)) return rc;
    const size_t last = t->enc.size() - 1;
    hipLaunchKernelGGL(bce_head_kernel, rows, rt, 0, st, t->ea[last], c.y_dim, t->ybatch, c.y_dim, c.y_dim, c.loss_eps, 1.0 / (double)B,
                       train ? t->eg[last] : nullptr, c.y_dim, t->rows, t->row_cnt);
    VN_CHECK_HIP(hipGetLastError());
    if (train)
      if (int rc = backward_net(t, t->enc, t->ea, t->eg, t->x_in, t->in0, nullptr, 0, B, st)) return rc;
    hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), rt, 0, st, t->rows, nullptr, t->row_cnt, B, losses);
    VN_CHECK_HIP(hipGetLastError());
  } else {
    if (c.kind == VAENMF_TRAIN_M2) {      // [x | y] for the encoder, y again beside z for the decoder
      hipLaunchKernelGGL(train_gather_kernel, rows, rt, 0, st, Y, (int64_t)ldy, NT, idx, c.y_dim, nullptr, nullptr, 0.0f, t->x_in, t->in0, c.x_dim);
      VN_CHECK_HIP(hipGetLastError());
      hipLaunchKernelGGL(train_gather_kernel, rows, rt, 0, st, Y, (int64_t)ldy, NT, idx, c.y_dim, nullptr, nullptr, 0.0f, t->d_in, t->d0, c.z_dim);
      VN_CHECK_HIP(hipGetLastError());
    }
    if (int rc = forward_net(t, t->enc, t->ea, t->x_in, t->in0, B, st)) return rc;
    if (!eps) {
      const uint32_t key = (uint32_t)(t->step + 1) ^ (train ? 0u : 0x80000000u);      // an evaluation does not draw a training step's noise
      if (int rc = launch_eps(seed, key, B, c.z_dim, t->eps, st)) return rc;
      eps = t->eps;
    }
    const float* ML = t->ea[t->enc.size() - 1];
    hipLaunchKernelGGL(latent_fwd_kernel, rows, dim3(64), 0, st, ML, 2 * c.z_dim, eps, c.z_dim, t->d_in, t->d0);
    VN_CHECK_HIP(hipGetLastError());
    if (int rc = forward_net(t, t->dec, t->da, t->d_in, t->d0, B, st)) return rc;
    const size_t dl = t->dec.size() - 1, el = t->enc.size() - 1;
    hipLaunchKernelGGL(elbo_out_kernel, rows, rt, 0, st, t->x_in, t->in0, t->da[dl], c.x_dim, c.x_dim, c.loss_eps, inv_b,
                       train ? t->dg[dl] : nullptr, c.x_dim, t->rows);
    VN_CHECK_HIP(hipGetLastError());
    if (train)
      if (int rc = backward_net(t, t->dec, t->da, t->dg, t->d_in, t->d0, t->d_in_g, c.z_dim, B, st)) return rc;
    hipLaunchKernelGGL(latent_bwd_kernel, rows, dim3(64), 0, st, ML, 2 * c.z_dim, eps, t->d_in_g, c.z_dim, c.z_dim, inv_b,
                       train ? t->eg[el] : nullptr, 2 * c.z_dim, t->rows + c.max_batch);
    VN_CHECK_HIP(hipGetLastError());
    if (train)
      if (int rc = backward_net(t, t->enc, t->ea, t->eg, t->x_in, t->in0, nullptr, 0, B, st)) return rc;
    hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), rt, 0, st, t->rows, t->rows + c.max_batch, nullptr, B, losses);
    VN_CHECK_HIP(hipGetLastError());
  }
  if (train) {
    t->step += 1;
    if (int rc = vaenmf_adam(t->P(), t->G(), t->Mo(), t->Vo(), (int64_t)t->n_params, t->step, c.lr, c.beta1, c.beta2, c.adam_eps, st)) return rc;
  }
  return 0;
}

}  // namespace

// ---- the building blocks on their own ----
#define TR_DIMS_OK(fn, M, in, out)                                                                                     \
  VN_REQUIRE((M) >= 1 && (M) <= TR_MAX_BATCH && (in) >= 1 && (in) <= TR_MAX_DIM && (out) >= 1 && (out) <= TR_MAX_DIM, \
             fn ": M=%d, in=%d, out=%d outside [1, %d] x [1, %d] x [1, %d]", M, in, out, TR_MAX_BATCH, TR_MAX_DIM, TR_MAX_DIM)
#define TR_ACT_OK(fn, act)                                                                                                              \
  VN_REQUIRE((act) == VAENMF_ACT_NONE || (act) == VAENMF_ACT_TANH || (act) == VAENMF_ACT_RELU || (act) == VAENMF_ACT_SIGMOID ||         \
                 (act) == VAENMF_ACT_EXP,                                                                                               \
             fn ": activation %d is not one of none, tanh, relu, sigmoid, exp", act)

extern "C" int vaenmf_train_dense_fwd(const float* X, int32_t M, int32_t in, int32_t ldx, const float* W, int32_t ldw, const float* b,
                                      int32_t out, int32_t act, float* Y, int32_t ldy, void* stream) {
  TR_DIMS_OK("vaenmf_train_dense_fwd", M, in, out);
  TR_ACT_OK("vaenmf_train_dense_fwd", act);
  VN_REQUIRE(X && W && Y, "vaenmf_train_dense_fwd: null X / W / Y");
  VN_REQUIRE(ldx >= in && ldw >= in && ldy >= out, "vaenmf_train_dense_fwd: ldx=%d, ldw=%d < in=%d or ldy=%d < out=%d", ldx, ldw, in, ldy, out);
  return gemm_fwd(X, M, in, ldx, W, ldw, b, out, act, Y, ldy, (hipStream_t)stream);
}

extern "C" int vaenmf_train_dense_dx(const float* dZ, int32_t M, int32_t out, int32_t ldz, const float* W, int32_t ldw, int32_t in,
                                     const float* Yprev, int32_t ldp, int32_t act, float* dX, int32_t lddx, void* stream) {
  TR_DIMS_OK("vaenmf_train_dense_dx", M, in, out);
  TR_ACT_OK("vaenmf_train_dense_dx", act);
  VN_REQUIRE(dZ && W && dX, "vaenmf_train_dense_dx: null dZ / W / dX");
  VN_REQUIRE(ldz >= out && ldw >= in && lddx >= in, "vaenmf_train_dense_dx: ldz=%d < out=%d or ldw=%d, lddx=%d < in=%d", ldz, out, ldw, lddx, in);
  VN_REQUIRE(act == VAENMF_ACT_NONE || (Yprev && ldp >= in), "vaenmf_train_dense_dx: an activation needs Yprev with ldp=%d >= in=%d", ldp, in);
  return gemm_dx(dZ, M, out, ldz, W, ldw, in, act == VAENMF_ACT_NONE ? nullptr : Yprev, ldp, act, dX, lddx, (hipStream_t)stream);
}

extern "C" int vaenmf_train_dense_dw(const float* dZ, int32_t M, int32_t out, int32_t ldz, const float* X, int32_t in, int32_t ldx,
                                     float* dW, int32_t lddw, float* db, void* stream) {
  TR_DIMS_OK("vaenmf_train_dense_dw", M, in, out);
  VN_REQUIRE(dZ && X && dW, "vaenmf_train_dense_dw: null dZ / X / dW");
  VN_REQUIRE(ldz >= out && ldx >= in && lddw >= in, "vaenmf_train_dense_dw: ldz=%d < out=%d or ldx=%d, lddw=%d < in=%d", ldz, out, ldx, lddw, in);
  return gemm_dw(dZ, M, out, ldz, X, in, ldx, dW, lddw, db, (hipStream_t)stream);
}

extern "C" int vaenmf_elbo_out(const float* X, int32_t ldx, const float* A, int32_t lda, int32_t B, int32_t F, double eps, float* dA,
                               int32_t ldd, double* row_recon, void* stream) {
  VN_REQUIRE(B >= 1 && B <= TR_MAX_BATCH && F >= 1 && F <= TR_MAX_DIM, "vaenmf_elbo_out: B=%d, F=%d", B, F);
  VN_REQUIRE(X && A && row_recon && ((uintptr_t)row_recon & 7) == 0, "vaenmf_elbo_out: null X / A / row_recon, or row_recon not aligned to 8 bytes");
  VN_REQUIRE(ldx >= F && lda >= F && (!dA || ldd >= F), "vaenmf_elbo_out: ldx=%d, lda=%d, ldd=%d < F=%d", ldx, lda, ldd, F);
  hipLaunchKernelGGL(elbo_out_kernel, dim3((unsigned)B), dim3(ROW_THREADS), 0, (hipStream_t)stream, X, ldx, A, lda, F, eps, 1.0f / (float)B, dA,
                     ldd, row_recon);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int vaenmf_elbo_latent_fwd(const float* ML, int32_t ldm, const float* eps, int32_t B, int32_t z, float* Z, int32_t ldz, void* stream) {
  VN_REQUIRE(B >= 1 && B <= TR_MAX_BATCH && z >= 1 && z <= TR_MAX_DIM / 2, "vaenmf_elbo_latent_fwd: B=%d, z=%d", B, z);
  VN_REQUIRE(ML && eps && Z && ldm >= 2 * z && ldz >= z, "vaenmf_elbo_latent_fwd: null buffers, ldm=%d < 2 z=%d or ldz=%d < z", ldm, 2 * z, ldz);
  hipLaunchKernelGGL(latent_fwd_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, ML, ldm, eps, z, Z, ldz);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int vaenmf_elbo_latent_bwd(const float* ML, int32_t ldm, const float* eps, const float* dZ, int32_t lddz, int32_t B, int32_t z,
                                      float* dML, int32_t lddm, double* row_kl, void* stream) {
  VN_REQUIRE(B >= 1 && B <= TR_MAX_BATCH && z >= 1 && z <= TR_MAX_DIM / 2, "vaenmf_elbo_latent_bwd: B=%d, z=%d", B, z);
  VN_REQUIRE(ML && row_kl && ldm >= 2 * z && ((uintptr_t)row_kl & 7) == 0, "vaenmf_elbo_latent_bwd: null ML / row_kl, ldm=%d < 2 z=%d, or row_kl not aligned",
             ldm, 2 * z);
  VN_REQUIRE(!dML || (eps && dZ && lddz >= z && lddm >= 2 * z), "vaenmf_elbo_latent_bwd: gradients need eps, dZ (lddz=%d >= z) and lddm=%d >= 2 z", lddz, lddm);
  hipLaunchKernelGGL(latent_bwd_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, ML, ldm, eps, dZ, lddz, z, 1.0f / (float)B, dML, lddm,
                     row_kl);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int vaenmf_bce_head(const float* A, int32_t lda, const float* Y, int32_t ldy, int32_t B, int32_t D, double eps, float* dA, int32_t ldd,
                               double* row_loss, int32_t* row_cnt, void* stream) {
  VN_REQUIRE(B >= 1 && B <= TR_MAX_BATCH && D >= 1 && D <= TR_MAX_DIM, "vaenmf_bce_head: B=%d, D=%d", B, D);
  VN_REQUIRE(A && Y && row_loss && row_cnt && ((uintptr_t)row_loss & 7) == 0, "vaenmf_bce_head: null buffers, or row_loss not aligned to 8 bytes");
  VN_REQUIRE(lda >= D && ldy >= D && (!dA || ldd >= D), "vaenmf_bce_head: lda=%d, ldy=%d, ldd=%d < D=%d", lda, ldy, ldd, D);
  hipLaunchKernelGGL(bce_head_kernel, dim3((unsigned)B), dim3(ROW_THREADS), 0, (hipStream_t)stream, A, lda, Y, ldy, D, eps, 1.0 / (double)B, dA, ldd,
                     row_loss, row_cnt);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int vaenmf_loss_reduce(const double* row_a, const double* row_b, const int32_t* row_cnt, int32_t B, double* out, void* stream) {
  VN_REQUIRE(B >= 1 && B <= TR_MAX_BATCH, "vaenmf_loss_reduce: B=%d", B);
  VN_REQUIRE(row_a && out && ((uintptr_t)out & 7) == 0 && ((uintptr_t)row_a & 7) == 0 && ((uintptr_t)row_b & 7) == 0,
             "vaenmf_loss_reduce: null row_a / out, or a buffer not aligned to 8 bytes");
  hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(ROW_THREADS), 0, (hipStream_t)stream, row_a, row_b, row_cnt, B, out);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int vaenmf_adam(float* p, const float* g, float* m, float* v, int64_t n, int64_t step, double lr, double beta1, double beta2,
                           double eps, void* stream) {
  VN_REQUIRE(n >= 0 && n <= ((int64_t)1 << 38), "vaenmf_adam: n=%lld", (long long)n);
  VN_REQUIRE(step >= 1, "vaenmf_adam: step=%lld, the first step is 1", (long long)step);
  VN_REQUIRE(lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0,
             "vaenmf_adam: lr=%g, betas=(%g, %g), eps=%g", lr, beta1, beta2, eps);
  if (n == 0) return 0;
  VN_REQUIRE(p && g && m && v, "vaenmf_adam: null buffers");
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  const double step_size = lr / bc1, bc2_sqrt = sqrt(bc2);
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, (float)(1.0 - beta1),
                     (float)beta2, (float)(1.0 - beta2), (float)(-step_size), (float)bc2_sqrt, (float)eps);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int vaenmf_train_gather(const float* src, int32_t lds, int64_t NT, const int32_t* idx, int32_t B, int32_t ncol, const float* mean,
                                   const float* std, float eps, float* dst, int32_t ldd, int32_t col0, void* stream) {
  VN_REQUIRE(B >= 1 && B <= TR_MAX_BATCH && ncol >= 1 && ncol <= TR_MAX_DIM, "vaenmf_train_gather: B=%d, ncol=%d", B, ncol);
  VN_REQUIRE(NT >= 1 && NT <= INT32_MAX, "vaenmf_train_gather: NT=%lld outside [1, 2^31)", (long long)NT);
  VN_REQUIRE(src && idx && dst, "vaenmf_train_gather: null src / idx / dst");
  VN_REQUIRE(lds >= ncol && col0 >= 0 && ldd >= col0 + ncol, "vaenmf_train_gather: lds=%d < ncol=%d, or columns [%d, %d) outside ldd=%d", lds, ncol,
             col0, col0 + ncol, ldd);
  VN_REQUIRE((mean == nullptr) == (std == nullptr), "vaenmf_train_gather: mean and std go together");
  hipLaunchKernelGGL(train_gather_kernel, dim3((unsigned)B), dim3(ROW_THREADS), 0, (hipStream_t)stream, src, (int64_t)lds, NT, idx, ncol, mean, std,
                     eps, dst, ldd, col0);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int vaenmf_train_eps_fill(uint64_t seed, int64_t step, int32_t B, int32_t z, float* eps_out, void* stream) {
  VN_REQUIRE(B >= 1 && B <= TR_MAX_BATCH && z >= 4 && z <= TR_MAX_DIM / 2 && z % 4 == 0, "vaenmf_train_eps_fill: B=%d, z=%d (a multiple of 4)", B, z);
  VN_REQUIRE(step >= 1 && step < ((int64_t)1 << 31), "vaenmf_train_eps_fill: step=%lld outside [1, 2^31)", (long long)step);
  VN_REQUIRE(eps_out, "vaenmf_train_eps_fill: null eps_out");
  return launch_eps(seed, (uint32_t)step, B, z, eps_out, (hipStream_t)stream);
}

// ---- the trainer ----
extern "C" int vaenmf_trainer_create(const vaenmf_trainer_config* cfg, vaenmf_trainer** out) {
  VN_REQUIRE(cfg && out, "vaenmf_trainer_create: null argument");
  *out = nullptr;
  const vaenmf_trainer_config& c = *cfg;
  VN_REQUIRE(c.kind == VAENMF_TRAIN_M1 || c.kind == VAENMF_TRAIN_M2 || c.kind == VAENMF_TRAIN_CLASSIFIER, "vaenmf_trainer_create: kind=%d", c.kind);
  VN_REQUIRE(c.x_dim >= 1 && c.x_dim <= TR_MAX_DIM, "vaenmf_trainer_create: x_dim=%d outside [1, %d]", c.x_dim, TR_MAX_DIM);
  VN_REQUIRE(c.n_hidden == 1 || c.n_hidden == 2, "vaenmf_trainer_create: %d hidden layers (one or two)", c.n_hidden);
  for (int i = 0; i < c.n_hidden; ++i)
    VN_REQUIRE(c.hidden[i] >= 1 && c.hidden[i] <= TR_MAX_DIM, "vaenmf_trainer_create: hidden[%d]=%d outside [1, %d]", i, c.hidden[i], TR_MAX_DIM);
  VN_REQUIRE(c.max_batch >= 1 && c.max_batch <= TR_MAX_BATCH, "vaenmf_trainer_create: max_batch=%d outside [1, %d]", c.max_batch, TR_MAX_BATCH);
  if (c.kind == VAENMF_TRAIN_M1) VN_REQUIRE(c.y_dim == 0, "vaenmf_trainer_create: M1 has no labels (y_dim=%d)", c.y_dim);
  else VN_REQUIRE(c.y_dim >= 1 && c.y_dim <= TR_MAX_DIM - c.x_dim, "vaenmf_trainer_create: y_dim=%d outside [1, %d]", c.y_dim, TR_MAX_DIM - c.x_dim);
  if (c.kind != VAENMF_TRAIN_CLASSIFIER)
    VN_REQUIRE(c.z_dim >= 4 && c.z_dim % 4 == 0 && c.z_dim <= 1024, "vaenmf_trainer_create: z_dim=%d (a multiple of 4 in [4, 1024])", c.z_dim);
  VN_REQUIRE(c.lr >= 0.0 && c.beta1 >= 0.0 && c.beta1 < 1.0 && c.beta2 >= 0.0 && c.beta2 < 1.0 && c.adam_eps >= 0.0 && c.loss_eps >= 0.0,
             "vaenmf_trainer_create: lr=%g, betas=(%g, %g), adam_eps=%g, loss_eps=%g", c.lr, c.beta1, c.beta2, c.adam_eps, c.loss_eps);
  vaenmf_trainer* t = new (std::nothrow) vaenmf_trainer();
  VN_REQUIRE(t, "vaenmf_trainer_create: out of host memory");
  t->cfg = c;
  const int nh = c.n_hidden;
  if (c.kind == VAENMF_TRAIN_CLASSIFIER) {
    t->in0 = c.x_dim;
    int in = t->in0;
    for (int i = 0; i < nh; ++i) { add_layer(t, t->enc, in, c.hidden[i], VAENMF_ACT_RELU, false); in = c.hidden[i]; }
    add_layer(t, t->enc, in, c.y_dim, VAENMF_ACT_NONE, false);         // the head applies the sigmoid
  } else {
    t->in0 = c.x_dim + c.y_dim; t->d0 = c.z_dim + c.y_dim;
    int in = t->in0;
    for (int i = 0; i < nh; ++i) { add_layer(t, t->enc, in, c.hidden[i], VAENMF_ACT_TANH, false); in = c.hidden[i]; }
    add_layer(t, t->enc, in, 2 * c.z_dim, VAENMF_ACT_NONE, true);
    in = t->d0;
    for (int i = nh - 1; i >= 0; --i) { add_layer(t, t->dec, in, c.hidden[i], VAENMF_ACT_TANH, false); in = c.hidden[i]; }    // reversed(h_dim)
    add_layer(t, t->dec, in, c.x_dim, VAENMF_ACT_NONE, false);         // the head applies the exponential
  }
  // activations: x_in, d_in, d_in_g, ybatch, then output and gradient of every layer
  const size_t mb = (size_t)c.max_batch;
  size_t n_act = mb * ((size_t)t->in0 + 2 * (size_t)t->d0 + (size_t)c.y_dim);
  for (const Layer& l : t->enc) n_act += 2 * mb * l.out;
  for (const Layer& l : t->dec) n_act += 2 * mb * l.out;
  const size_t n_eps = mb * (size_t)(c.z_dim > 0 ? c.z_dim : 1);
  if (hipMalloc(&t->arena, 4 * t->n_params * sizeof(float)) != hipSuccess || hipMalloc(&t->act, (n_act + n_eps) * sizeof(float)) != hipSuccess ||
      hipMalloc(&t->rows, 2 * mb * sizeof(double)) != hipSuccess || hipMalloc(&t->row_cnt, 4 * mb * sizeof(int32_t)) != hipSuccess) {
    vaenmf_set_error("vaenmf_trainer_create: device allocation failed");
    vaenmf_trainer_destroy(t);
    return -2;
  }
  g_vn_dev_allocs += 4;
  if (hipMemset(t->arena, 0, 4 * t->n_params * sizeof(float)) != hipSuccess || hipMemset(t->act, 0, (n_act + n_eps) * sizeof(float)) != hipSuccess ||
      hipMemset(t->rows, 0, 2 * mb * sizeof(double)) != hipSuccess || hipMemset(t->row_cnt, 0, 4 * mb * sizeof(int32_t)) != hipSuccess) {
    vaenmf_set_error("vaenmf_trainer_create: hipMemset failed");
    vaenmf_trainer_destroy(t);
    return -2;
  }
  float* a = t->act;
  t->x_in = a; a += mb * t->in0;
  t->d_in = a; a += mb * t->d0;
  t->d_in_g = a; a += mb * t->d0;
  t->ybatch = a; a += mb * c.y_dim;
  for (const Layer& l : t->enc) { t->ea.push_back(a); a += mb * l.out; t->eg.push_back(a); a += mb * l.out; }
  for (const Layer& l : t->dec) { t->da.push_back(a); a += mb * l.out; t->dg.push_back(a); a += mb * l.out; }
  t->eps = a;
  *out = t;
  return 0;
}

extern "C" void vaenmf_trainer_destroy(vaenmf_trainer* t) {
  if (!t) return;
  (void)hipFree(t->arena); (void)hipFree(t->act); (void)hipFree(t->rows); (void)hipFree(t->row_cnt);
  delete t;
}

extern "C" int vaenmf_trainer_num_tensors(const vaenmf_trainer* t) {
  if (!t) { vaenmf_set_error("vaenmf_trainer_num_tensors: null trainer"); return -1; }
  return (int)t->tensors.size();
}

extern "C" int vaenmf_trainer_tensor_shape(const vaenmf_trainer* t, int32_t i, int32_t* rows, int32_t* cols) {
  VN_REQUIRE(t && rows && cols, "vaenmf_trainer_tensor_shape: null argument");
  VN_REQUIRE(i >= 0 && i < (int)t->tensors.size(), "vaenmf_trainer_tensor_shape: tensor %d of %d", i, (int)t->tensors.size());
  *rows = t->tensors[i].rows; *cols = t->tensors[i].cols;
  return 0;
}

static int tensor_span(const char* fn, const vaenmf_trainer* t, int32_t which, int32_t i, size_t* off, size_t* n) {
  VN_REQUIRE(t != nullptr, "%s: null trainer", fn);
  VN_REQUIRE(which >= VAENMF_TRAIN_PARAM && which <= VAENMF_TRAIN_ADAM_V, "%s: which=%d", fn, which);
  VN_REQUIRE(i >= 0 && i < (int)t->tensors.size(), "%s: tensor %d of %d", fn, i, (int)t->tensors.size());
  const Tensor& e = t->tensors[i];
  *off = (size_t)which * t->n_params + e.off;
  *n = (size_t)e.rows * (e.cols ? e.cols : 1);
  return 0;
}

extern "C" int vaenmf_trainer_set_tensor(vaenmf_trainer* t, int32_t which, int32_t i, const float* src, void* stream) {
  size_t off, n;
  if (int rc = tensor_span("vaenmf_trainer_set_tensor", t, which, i, &off, &n)) return rc;
  VN_REQUIRE(src, "vaenmf_trainer_set_tensor: null src");
  VN_CHECK_HIP(hipMemcpyAsync(t->arena + off, src, n * sizeof(float), hipMemcpyDefault, (hipStream_t)stream));
  return 0;
}

extern "C" int vaenmf_trainer_get_tensor(const vaenmf_trainer* t, int32_t which, int32_t i, float* dst, void* stream) {
  size_t off, n;
  if (int rc = tensor_span("vaenmf_trainer_get_tensor", t, which, i, &off, &n)) return rc;
  VN_REQUIRE(dst, "vaenmf_trainer_get_tensor: null dst");
  VN_CHECK_HIP(hipMemcpyAsync(dst, t->arena + off, n * sizeof(float), hipMemcpyDefault, (hipStream_t)stream));
  return 0;
}

extern "C" int vaenmf_trainer_set_params(vaenmf_trainer* t, int32_t i, const float* src, void* stream) {
  return vaenmf_trainer_set_tensor(t, VAENMF_TRAIN_PARAM, i, src, stream);
}
extern "C" int vaenmf_trainer_get_params(const vaenmf_trainer* t, int32_t i, float* dst, void* stream) {
  return vaenmf_trainer_get_tensor(t, VAENMF_TRAIN_PARAM, i, dst, stream);
}

extern "C" int vaenmf_trainer_set_norm(vaenmf_trainer* t, const float* mean, const float* std, float eps) {
  VN_REQUIRE(t != nullptr, "vaenmf_trainer_set_norm: null trainer");
  VN_REQUIRE(t->cfg.kind == VAENMF_TRAIN_CLASSIFIER, "vaenmf_trainer_set_norm: only the classifier normalises its input");
  VN_REQUIRE((mean == nullptr) == (std == nullptr), "vaenmf_trainer_set_norm: mean and std go together");
  t->mean = mean; t->std = std; t->norm_eps = eps;
  return 0;
}

extern "C" int64_t vaenmf_trainer_step_count(const vaenmf_trainer* t) {
  if (!t) { vaenmf_set_error("vaenmf_trainer_step_count: null trainer"); return -1; }
  return t->step;
}

extern "C" int vaenmf_trainer_set_step_count(vaenmf_trainer* t, int64_t step) {
  VN_REQUIRE(t != nullptr, "vaenmf_trainer_set_step_count: null trainer");
  VN_REQUIRE(step >= 0 && step < ((int64_t)1 << 31) - 1, "vaenmf_trainer_set_step_count: step=%lld outside [0, 2^31 - 1)", (long long)step);
  t->step = step;
  return 0;
}

extern "C" int vaenmf_trainer_step(vaenmf_trainer* t, const float* X, int32_t ldx, const float* Y, int32_t ldy, int64_t NT, const int32_t* idx,
                                   int32_t B, const float* eps, uint64_t seed, double* losses, void* stream) {
  if (int rc = check_step_args("vaenmf_trainer_step", t, X, ldx, Y, ldy, NT, idx, B, losses)) return rc;
  VN_REQUIRE(t->step < ((int64_t)1 << 31) - 2, "vaenmf_trainer_step: step counter exhausted");
  return run_step(t, true, X, ldx, Y, ldy, NT, idx, B, eps, seed, losses, (hipStream_t)stream);
}

extern "C" int vaenmf_trainer_eval(vaenmf_trainer* t, const float* X, int32_t ldx, const float* Y, int32_t ldy, int64_t NT, const int32_t* idx,
                                   int32_t B, const float* eps, uint64_t seed, double* losses, void* stream) {
  if (int rc = check_step_args("vaenmf_trainer_eval", t, X, ldx, Y, ldy, NT, idx, B, losses)) return rc;
  return run_step(t, false, X, ldx, Y, ldy, NT, idx, B, eps, seed, losses, (hipStream_t)stream);
}

extern "C" int vaenmf_trainer_eps_fill(const vaenmf_trainer* t, int64_t step, int32_t B, uint64_t seed, float* eps_out, void* stream) {
  VN_REQUIRE(t != nullptr, "vaenmf_trainer_eps_fill: null trainer");
  VN_REQUIRE(t->cfg.kind != VAENMF_TRAIN_CLASSIFIER, "vaenmf_trainer_eps_fill: the classifier draws nothing");
  VN_REQUIRE(B >= 1 && B <= t->cfg.max_batch, "vaenmf_trainer_eps_fill: B=%d outside [1, max_batch=%d]", B, t->cfg.max_batch);
  return vaenmf_train_eps_fill(seed, step, B, t->cfg.z_dim, eps_out, stream);
}
