// Training the supervised Wiener-mask baseline (scripts/training_wiener_filter.py:76-188) on the device: the reference's
// Classifier with up to eight relu layers and F sigmoid outputs under one of the three mean-squared-error losses of
// python/models/utils.py:93-104.  include/vaenmf_mask.h states the contracts.
//
// New here: the MSE head and a trainer that holds any number of layers.  The dense layers, the gather, Adam and the loss
// reduction are train.hip's, called through their public launchers (include/vaenmf.h), so a step keeps their fixed
// summation order: k-ordered fmaf chains, one workgroup per reduction, no atomics.  The head sums a row in double, lanes by
// the xor butterfly and waves in wave order, as the BCE head does.
#include <math.h>
#include <new>
#include <vector>
#include "common.h"
#include "../../include/vaenmf_mask.h"

namespace {

constexpr int MK_THREADS = 256;
constexpr int MK_MAX_DIM = 4096, MK_MAX_BATCH = 65536;

__device__ __forceinline__ double mk_block_sum(double v, double* red) {     // thread 0's value is the sum
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = red[0];
#pragma unroll
  for (int i = 1; i < MK_THREADS / 64; ++i) r += red[i];
  return r;
}

// one workgroup per row; the terms are evaluated in double from the float pre-activation, labels and power
template <int LOSS>
__global__ __launch_bounds__(MK_THREADS) void mse_head_kernel(const float* __restrict__ A, int lda, const float* __restrict__ Y, int ldy,
                                                              const float* __restrict__ P, int ldp, int D, double inv_b,
                                                              float* __restrict__ dA, int ldd, double* __restrict__ row_loss) {
  __shared__ double red[MK_THREADS / 64];
  const int b = blockIdx.x;
  double s = 0.0;
  for (int j = threadIdx.x; j < D; j += MK_THREADS) {
    const double a = (double)A[(int64_t)b * lda + j], y = (double)Y[(int64_t)b * ldy + j];
    // yh = sigmoid(a) and q = 1 - yh = sigmoid(-a), each from the exponential that does not overflow
    const double e = exp(-fabs(a));
    const double big = 1.0 / (1.0 + e), small = e / (1.0 + e);
    const double yh = a >= 0.0 ? big : small, q = a >= 0.0 ? small : big;
    double r, w;                                  // the term is r^2, its derivative by yh is -2 r w
    if (LOSS == VAENMF_MSE_MASK) {
      r = y - yh; w = 1.0;
    } else {
      const double x = sqrt((double)P[(int64_t)b * ldp + j]);
      if (LOSS == VAENMF_MSE_SIGNAL) { r = (y - yh) * x; w = x; }
      else { r = y - yh * x; w = x; }
    }
    s += r * r;
    if (dA) dA[(int64_t)b * ldd + j] = (float)(-2.0 * r * w * (yh * q) * inv_b);
  }
  s = mk_block_sum(s, red);
  if (threadIdx.x == 0) row_loss[b] = s;
}

struct Layer {
  int in, out, act;
  size_t w, b;           // offsets into the parameter arena (floats): W [out][in], b [out]
};
struct Tensor {          // a tensor of the state_dict, in its order
  size_t off; int rows, cols;
};

}  // namespace

struct vaenmf_mask_trainer {
  vaenmf_mask_trainer_config cfg;
  std::vector<Layer> net;         // hidden layers (relu), then the output layer (the head applies the sigmoid)
  std::vector<Tensor> tensors;
  size_t n_params = 0;
  float* arena = nullptr;         // [4][n_params]: parameters, gradients, Adam m, Adam v
  float* act = nullptr;           // x_in, p_raw (signal / msa only), ybatch, then output and gradient of every layer ([max_batch][width] each)
  double* rows = nullptr;         // [max_batch] per-row loss sums
  const float *mean = nullptr, *std = nullptr;
  float norm_eps = 0.0f;
  float *x_in = nullptr, *p_raw = nullptr, *ybatch = nullptr;
  std::vector<float*> out, grad;
  int64_t step = 0;
  float* P() const { return arena; }
  float* G() const { return arena + n_params; }
  float* Mo() const { return arena + 2 * n_params; }
  float* Vo() const { return arena + 3 * n_params; }
};

namespace {

int check_step_args(const char* fn, const vaenmf_mask_trainer* t, const float* X, int32_t ldx, const float* Y, int32_t ldy, int64_t NT,
                    const int32_t* idx, int32_t B, const double* losses) {
  VN_REQUIRE(t != nullptr, "%s: null trainer", fn);
  const vaenmf_mask_trainer_config& c = t->cfg;
  VN_REQUIRE(B >= 1 && B <= c.max_batch, "%s: B=%d outside [1, max_batch=%d]", fn, B, c.max_batch);
  VN_REQUIRE(NT >= 1 && NT <= INT32_MAX, "%s: NT=%lld outside [1, 2^31)", fn, (long long)NT);
  VN_REQUIRE(X && Y && idx && losses, "%s: null X / Y / idx / losses", fn);
  VN_REQUIRE(ldx >= c.x_dim, "%s: ldx=%d < x_dim=%d", fn, ldx, c.x_dim);
  VN_REQUIRE(ldy >= c.y_dim, "%s: ldy=%d < y_dim=%d", fn, ldy, c.y_dim);
  VN_REQUIRE(((uintptr_t)losses & 7) == 0, "%s: losses must be aligned to 8 bytes", fn);
  return 0;
}

// forward and loss (and, with train, backward and Adam) of one batch
int run_step(vaenmf_mask_trainer* t, bool train, const float* X, int32_t ldx, const float* Y, int32_t ldy, int64_t NT, const int32_t* idx,
             int32_t B, double* losses, void* st) {
  const vaenmf_mask_trainer_config& c = t->cfg;
  if (int rc = vaenmf_train_gather(X, ldx, NT, idx, B, c.x_dim, t->mean, t->std, t->norm_eps, t->x_in, c.x_dim, 0, st)) return rc;
  if (int rc = vaenmf_train_gather(Y, ldy, NT, idx, B, c.y_dim, nullptr, nullptr, 0.0f, t->ybatch, c.y_dim, 0, st)) return rc;
  const float* praw = nullptr;
  if (c.loss != VAENMF_MSE_MASK) {
    praw = t->x_in;              // without a normalisation the input rows are the power rows
    if (t->mean) {
      if (int rc = vaenmf_train_gather(X, ldx, NT, idx, B, c.x_dim, nullptr, nullptr, 0.0f, t->p_raw, c.x_dim, 0, st)) return rc;
      praw = t->p_raw;
    }
  }
  const size_t n = t->net.size(), last = n - 1;
  for (size_t i = 0; i < n; ++i) {
    const Layer& l = t->net[i];
    if (int rc = vaenmf_train_dense_fwd(i ? t->out[i - 1] : t->x_in, B, l.in, l.in, t->P() + l.w, l.in, t->P() + l.b, l.out, l.act, t->out[i],
                                        l.out, st))
      return rc;
  }
  if (int rc = vaenmf_mse_head(t->out[last], c.y_dim, t->ybatch, c.y_dim, praw, c.x_dim, B, c.y_dim, c.loss, train ? t->grad[last] : nullptr,
                               c.y_dim, t->rows, st))
    return rc;
  if (train) {
    for (size_t i = n; i-- > 0;) {
      const Layer& l = t->net[i];
      if (int rc = vaenmf_train_dense_dw(t->grad[i], B, l.out, l.out, i ? t->out[i - 1] : t->x_in, l.in, l.in, t->G() + l.w, l.in, t->G() + l.b, st))
        return rc;
      if (i)
        if (int rc = vaenmf_train_dense_dx(t->grad[i], B, l.out, l.out, t->P() + l.w, l.in, l.in, t->out[i - 1], l.in, t->net[i - 1].act,
                                           t->grad[i - 1], l.in, st))
          return rc;
    }
  }
  if (int rc = vaenmf_loss_reduce(t->rows, nullptr, nullptr, B, losses, st)) return rc;
  if (train) {
    t->step += 1;
    if (int rc = vaenmf_adam(t->P(), t->G(), t->Mo(), t->Vo(), (int64_t)t->n_params, t->step, c.lr, c.beta1, c.beta2, c.adam_eps, st)) return rc;
  }
  return 0;
}

int tensor_span(const char* fn, const vaenmf_mask_trainer* t, int32_t which, int32_t i, size_t* off, size_t* n) {
  VN_REQUIRE(t != nullptr, "%s: null trainer", fn);
  VN_REQUIRE(which >= VAENMF_MASK_PARAM && which <= VAENMF_MASK_ADAM_V, "%s: which=%d", fn, which);
  VN_REQUIRE(i >= 0 && i < (int)t->tensors.size(), "%s: tensor %d of %d", fn, i, (int)t->tensors.size());
  const Tensor& e = t->tensors[i];
  *off = (size_t)which * t->n_params + e.off;
  *n = (size_t)e.rows * (e.cols ? e.cols : 1);
  return 0;
}

}  // namespace

extern "C" int vaenmf_mse_head(const float* A, int32_t lda, const float* Y, int32_t ldy, const float* P, int32_t ldp, int32_t B, int32_t D,
                               int32_t loss, float* dA, int32_t ldd, double* row_loss, void* stream) {
  VN_REQUIRE(B >= 1 && B <= MK_MAX_BATCH && D >= 1 && D <= MK_MAX_DIM, "vaenmf_mse_head: B=%d, D=%d outside [1, %d] x [1, %d]", B, D, MK_MAX_BATCH,
             MK_MAX_DIM);
  VN_REQUIRE(loss == VAENMF_MSE_MASK || loss == VAENMF_MSE_SIGNAL || loss == VAENMF_MSE_MSA, "vaenmf_mse_head: loss=%d is not one of mask, signal, msa",
             loss);
  VN_REQUIRE(A && Y && row_loss && ((uintptr_t)row_loss & 7) == 0, "vaenmf_mse_head: null A / Y / row_loss, or row_loss not aligned to 8 bytes");
  VN_REQUIRE(lda >= D && ldy >= D && (!dA || ldd >= D), "vaenmf_mse_head: lda=%d, ldy=%d, ldd=%d < D=%d", lda, ldy, ldd, D);
  VN_REQUIRE(loss == VAENMF_MSE_MASK || (P && ldp >= D), "vaenmf_mse_head: the signal and msa losses need the power rows P with ldp=%d >= D=%d", ldp, D);
  const dim3 grid((unsigned)B), block(MK_THREADS);
  const double inv_b = 1.0 / (double)B;
  hipStream_t st = (hipStream_t)stream;
  if (loss == VAENMF_MSE_MASK) hipLaunchKernelGGL((mse_head_kernel<VAENMF_MSE_MASK>), grid, block, 0, st, A, lda, Y, ldy, P, ldp, D, inv_b, dA, ldd, row_loss);
  else if (loss == VAENMF_MSE_SIGNAL)
    hipLaunchKernelGGL((mse_head_kernel<VAENMF_MSE_SIGNAL>), grid, block, 0, st, A, lda, Y, ldy, P, ldp, D, inv_b, dA, ldd, row_loss);
  else hipLaunchKernelGGL((mse_head_kernel<VAENMF_MSE_MSA>), grid, block, 0, st, A, lda, Y, ldy, P, ldp, D, inv_b, dA, ldd, row_loss);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int vaenmf_mask_trainer_create(const vaenmf_mask_trainer_config* cfg, vaenmf_mask_trainer** out) {
  VN_REQUIRE(cfg && out, "vaenmf_mask_trainer_create: null argument");
  *out = nullptr;
  const vaenmf_mask_trainer_config& c = *cfg;
  VN_REQUIRE(c.x_dim >= 1 && c.x_dim <= MK_MAX_DIM, "vaenmf_mask_trainer_create: x_dim=%d outside [1, %d]", c.x_dim, MK_MAX_DIM);
  VN_REQUIRE(c.y_dim >= 1 && c.y_dim <= MK_MAX_DIM, "vaenmf_mask_trainer_create: y_dim=%d outside [1, %d]", c.y_dim, MK_MAX_DIM);
  VN_REQUIRE(c.n_hidden >= 1 && c.n_hidden <= VAENMF_MASK_MAX_HIDDEN, "vaenmf_mask_trainer_create: %d hidden layers (1 .. %d)", c.n_hidden,
             VAENMF_MASK_MAX_HIDDEN);
  for (int i = 0; i < c.n_hidden; ++i)
    VN_REQUIRE(c.hidden[i] >= 1 && c.hidden[i] <= MK_MAX_DIM, "vaenmf_mask_trainer_create: hidden[%d]=%d outside [1, %d]", i, c.hidden[i], MK_MAX_DIM);
  VN_REQUIRE(c.loss == VAENMF_MSE_MASK || c.loss == VAENMF_MSE_SIGNAL || c.loss == VAENMF_MSE_MSA,
             "vaenmf_mask_trainer_create: loss=%d is not one of mask, signal, msa", c.loss);
  VN_REQUIRE(c.loss == VAENMF_MSE_MASK || c.y_dim == c.x_dim, "vaenmf_mask_trainer_create: the signal and msa losses need y_dim=%d == x_dim=%d", c.y_dim,
             c.x_dim);
  VN_REQUIRE(c.max_batch >= 1 && c.max_batch <= MK_MAX_BATCH, "vaenmf_mask_trainer_create: max_batch=%d outside [1, %d]", c.max_batch, MK_MAX_BATCH);
  VN_REQUIRE(c.lr >= 0.0 && c.beta1 >= 0.0 && c.beta1 < 1.0 && c.beta2 >= 0.0 && c.beta2 < 1.0 && c.adam_eps >= 0.0,
             "vaenmf_mask_trainer_create: lr=%g, betas=(%g, %g), adam_eps=%g", c.lr, c.beta1, c.beta2, c.adam_eps);
  vaenmf_mask_trainer* t = new (std::nothrow) vaenmf_mask_trainer();
  VN_REQUIRE(t, "vaenmf_mask_trainer_create: out of host memory");
  t->cfg = c;
  int in = c.x_dim;
  for (int i = 0; i <= c.n_hidden; ++i) {
    Layer l;
    l.in = in; l.out = i < c.n_hidden ? c.hidden[i] : c.y_dim; l.act = i < c.n_hidden ? VAENMF_ACT_RELU : VAENMF_ACT_NONE;
    l.w = t->n_params; t->n_params += (size_t)l.in * l.out;
    l.b = t->n_params; t->n_params += (size_t)l.out;
    t->net.push_back(l);
    t->tensors.push_back({l.w, l.out, l.in}); t->tensors.push_back({l.b, l.out, 0});
    in = l.out;
  }
  const size_t mb = (size_t)c.max_batch;
  const size_t n_raw = c.loss != VAENMF_MSE_MASK ? mb * (size_t)c.x_dim : 0;      // the mask loss never reads the raw power rows
  size_t n_act = mb * ((size_t)c.x_dim + (size_t)c.y_dim) + n_raw;
  for (const Layer& l : t->net) n_act += 2 * mb * l.out;
  if (hipMalloc(&t->arena, 4 * t->n_params * sizeof(float)) != hipSuccess || hipMalloc(&t->act, n_act * sizeof(float)) != hipSuccess ||
      hipMalloc(&t->rows, mb * sizeof(double)) != hipSuccess) {
    vaenmf_set_error("vaenmf_mask_trainer_create: device allocation failed");
    vaenmf_mask_trainer_destroy(t);
    return -2;
  }
  g_vn_dev_allocs += 3;
  if (hipMemset(t->arena, 0, 4 * t->n_params * sizeof(float)) != hipSuccess || hipMemset(t->act, 0, n_act * sizeof(float)) != hipSuccess ||
      hipMemset(t->rows, 0, mb * sizeof(double)) != hipSuccess) {
    vaenmf_set_error("vaenmf_mask_trainer_create: hipMemset failed");
    vaenmf_mask_trainer_destroy(t);
    return -2;
  }
  float* a = t->act;
  t->x_in = a; a += mb * c.x_dim;
  t->p_raw = n_raw ? a : nullptr; a += n_raw;
  t->ybatch = a; a += mb * c.y_dim;
  for (const Layer& l : t->net) { t->out.push_back(a); a += mb * l.out; t->grad.push_back(a); a += mb * l.out; }
  *out = t;
  return 0;
}

extern "C" void vaenmf_mask_trainer_destroy(vaenmf_mask_trainer* t) {
  if (!t) return;
  (void)hipFree(t->arena); (void)hipFree(t->act); (void)hipFree(t->rows);
  delete t;
}

extern "C" int vaenmf_mask_trainer_num_tensors(const vaenmf_mask_trainer* t) {
  if (!t) { vaenmf_set_error("vaenmf_mask_trainer_num_tensors: null trainer"); return -1; }
  return (int)t->tensors.size();
}

extern "C" int vaenmf_mask_trainer_tensor_shape(const vaenmf_mask_trainer* t, int32_t i, int32_t* rows, int32_t* cols) {
  VN_REQUIRE(t && rows && cols, "vaenmf_mask_trainer_tensor_shape: null argument");
  VN_REQUIRE(i >= 0 && i < (int)t->tensors.size(), "vaenmf_mask_trainer_tensor_shape: tensor %d of %d", i, (int)t->tensors.size());
  *rows = t->tensors[i].rows; *cols = t->tensors[i].cols;
  return 0;
}

extern "C" int vaenmf_mask_trainer_set_tensor(vaenmf_mask_trainer* t, int32_t which, int32_t i, const float* src, void* stream) {
  size_t off, n;
  if (int rc = tensor_span("vaenmf_mask_trainer_set_tensor", t, which, i, &off, &n)) return rc;
  VN_REQUIRE(src, "vaenmf_mask_trainer_set_tensor: null src");
  VN_CHECK_HIP(hipMemcpyAsync(t->arena + off, src, n * sizeof(float), hipMemcpyDefault, (hipStream_t)stream));
  return 0;
}

extern "C" int vaenmf_mask_trainer_get_tensor(const vaenmf_mask_trainer* t, int32_t which, int32_t i, float* dst, void* stream) {
  size_t off, n;
  if (int rc = tensor_span("vaenmf_mask_trainer_get_tensor", t, which, i, &off, &n)) return rc;
  VN_REQUIRE(dst, "vaenmf_mask_trainer_get_tensor: null dst");
  VN_CHECK_HIP(hipMemcpyAsync(dst, t->arena + off, n * sizeof(float), hipMemcpyDefault, (hipStream_t)stream));
  return 0;
}

extern "C" int vaenmf_mask_trainer_set_norm(vaenmf_mask_trainer* t, const float* mean, const float* std, float eps) {
  VN_REQUIRE(t != nullptr, "vaenmf_mask_trainer_set_norm: null trainer");
  VN_REQUIRE((mean == nullptr) == (std == nullptr), "vaenmf_mask_trainer_set_norm: mean and std go together");
  t->mean = mean; t->std = std; t->norm_eps = eps;
  return 0;
}

extern "C" int64_t vaenmf_mask_trainer_step_count(const vaenmf_mask_trainer* t) {
  if (!t) { vaenmf_set_error("vaenmf_mask_trainer_step_count: null trainer"); return -1; }
  return t->step;
}

extern "C" int vaenmf_mask_trainer_set_step_count(vaenmf_mask_trainer* t, int64_t step) {
  VN_REQUIRE(t != nullptr, "vaenmf_mask_trainer_set_step_count: null trainer");
  VN_REQUIRE(step >= 0 && step < ((int64_t)1 << 31) - 1, "vaenmf_mask_trainer_set_step_count: step=%lld outside [0, 2^31 - 1)", (long long)step);
  t->step = step;
  return 0;
}

extern "C" int vaenmf_mask_trainer_step(vaenmf_mask_trainer* t, const float* X, int32_t ldx, const float* Y, int32_t ldy, int64_t NT,
                                        const int32_t* idx, int32_t B, double* losses, void* stream) {
  if (int rc = check_step_args("vaenmf_mask_trainer_step", t, X, ldx, Y, ldy, NT, idx, B, losses)) return rc;
  VN_REQUIRE(t->step < ((int64_t)1 << 31) - 2, "vaenmf_mask_trainer_step: step counter exhausted");
  return run_step(t, true, X, ldx, Y, ldy, NT, idx, B, losses, stream);
}

extern "C" int vaenmf_mask_trainer_eval(vaenmf_mask_trainer* t, const float* X, int32_t ldx, const float* Y, int32_t ldy, int64_t NT,
                                        const int32_t* idx, int32_t B, double* losses, void* stream) {
  if (int rc = check_step_args("vaenmf_mask_trainer_eval", t, X, ldx, Y, ldy, NT, idx, B, losses)) return rc;
  return run_step(t, false, X, ldx, Y, ldy, NT, idx, B, losses, stream);
}
