/* vaenmf_mask.h -- training the supervised Wiener-mask baseline (scripts/training_wiener_filter.py) on the device.
 *
 * A second public header of libvaenmf.so beside vaenmf.h, with the same conventions: every function returns 0 on success
 * or a negative code (-1: a refused argument, -2: a HIP error) and vaenmf_last_error() holds the message; DEV marks device
 * memory; rows carry leading dimensions, and columns between a row's width and its leading dimension are never read and
 * never written.
 *
 * The network is the reference's Classifier([x_dim, h_dim, y_dim], batch_norm = False): x -> hidden (relu) .. -> y_dim
 * sigmoid outputs (python/models/models.py:41-62) with up to eight hidden layers, trained with torch.optim.Adam on one of
 * the three mean-squared-error losses of python/models/utils.py:93-104.  The dense layers, the gather, Adam and the loss
 * reduction are those of vaenmf.h (vaenmf_train_dense_fwd / _dx / _dw, vaenmf_train_gather, vaenmf_adam,
 * vaenmf_loss_reduce) with their fixed summation order: the same inputs give the same bits in every run, no atomics, no
 * split reductions.
 *
 * Streams.  Everything is ordered on `stream`: every launch and every copy of a call goes to the stream it is given, and
 * nothing here synchronises except vaenmf_mask_trainer_create / _destroy.  A step reads its step number on the host for
 * Adam's bias corrections, so vaenmf_mask_trainer_step may not be captured into a graph: a replay would repeat the
 * corrections of the step that was captured.
 */
#ifndef VAENMF_MASK_H
#define VAENMF_MASK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The head.  a = the network's output BEFORE the sigmoid; yh = sigmoid(a) and 1 - yh = sigmoid(-a), each evaluated in
 * double from the exponential that does not overflow; x = sqrt(P) of the RAW power row P (not the normalised input).
 * B rows, one workgroup per row, the per-row sums in double:
 *   VAENMF_MSE_MASK    mean_square_error_mask:                 row[b] = sum_j (y - yh)^2,
 *                                                              dA = -2 (y - yh) yh (1 - yh) / B          (P may be NULL)
 *   VAENMF_MSE_SIGNAL  mean_square_error_signal(sqrt(x), ..):  row[b] = sum_j ((y - yh) x)^2,
 *                                                              dA = -2 (y - yh) x^2 yh (1 - yh) / B
 *   VAENMF_MSE_MSA     magnitude_spectrum_approxiamation_loss(sqrt(x), s = y, ..), y = |S|:
 *                                                              row[b] = sum_j (y - yh x)^2,
 *                                                              dA = -2 (y - yh x) x yh (1 - yh) / B
 * The loss is the mean of row over B (vaenmf_loss_reduce).  dA NULL: no gradient (evaluation).  A saturated output
 * (|a| about 40) has yh (1 - yh) of 4e-18 and so a gradient of zero in float32 terms, never a NaN; P = 0 is a legal input.
 * A DEV [B][lda], Y DEV [B][ldy], P DEV [B][ldp], dA DEV [B][ldd], row_loss DEV [B] double (8-byte aligned).
 * Refused with -1: B outside [1, 65536], D outside [1, 4096], a leading dimension below D, an unknown loss, P NULL for
 * SIGNAL / MSA. */
enum { VAENMF_MSE_MASK = 0, VAENMF_MSE_SIGNAL = 1, VAENMF_MSE_MSA = 2 };
int vaenmf_mse_head(const float* A, int32_t lda, const float* Y, int32_t ldy, const float* P, int32_t ldp, int32_t B, int32_t D,
                    int32_t loss, float* dA, int32_t ldd, double* row_loss, void* stream);

/* The trainer: the parameters, the gradients of the last step and Adam's m and v in one device arena, and the buffers of a
 * step.  Accepted: n_hidden in [1, 8]; x_dim, y_dim and every hidden width in [1, 4096]; max_batch in [1, 65536]; for the
 * losses SIGNAL and MSA y_dim == x_dim (they weigh output j with bin j of the input).  Anything else is refused with -1
 * and a message.
 * Tensors are numbered in the order of the reference's state_dict: hidden.i.weight [out][in], hidden.i.bias, ...,
 * output_layer.weight, output_layer.bias.  _tensor_shape gives rows and cols (cols = 0 for a bias).  set / get copy one
 * tensor (src / dst DEV or HOST, contiguous) asynchronously on `stream`; `which` is VAENMF_MASK_PARAM, _GRAD (of the last
 * step), _ADAM_M or _ADAM_V.
 * vaenmf_mask_trainer_step: one step on the rows idx[0..B) (DEV int32, each in [0, NT)) of X DEV [NT][ldx], the power
 *   frames, and Y DEV [NT][ldy], the labels:
 *     1. gather the input (x - mean) / (std + eps), or x itself when no normalisation is set, the label rows, and -- for
 *        SIGNAL / MSA under a normalisation -- the raw power rows,
 *     2. forward through the relu layers to the pre-sigmoid output a,
 *     3. vaenmf_mse_head,
 *     4. backward,
 *     5. one Adam update over the whole parameter arena (one launch),
 *     6. losses DEV, 64 bytes (8-byte aligned) as vaenmf_loss_reduce writes them: double {loss, loss, 0, 0}, then four
 *        int64 zeros.
 *   B in [1, max_batch].  The step's number (the first is 1) is read on the host: see `Streams` above.
 * vaenmf_mask_trainer_eval: steps 1 - 3 and 6 only; parameters, gradients, Adam state and the step count stay as they are.
 * vaenmf_mask_trainer_set_norm: mean, std DEV [x_dim], caller-owned, read at every step (NULL, NULL: no normalisation).
 * vaenmf_mask_trainer_set_step_count: resume; step in [0, 2^31 - 1). */
typedef struct vaenmf_mask_trainer vaenmf_mask_trainer;
enum { VAENMF_MASK_PARAM = 0, VAENMF_MASK_GRAD = 1, VAENMF_MASK_ADAM_M = 2, VAENMF_MASK_ADAM_V = 3 };
enum { VAENMF_MASK_MAX_HIDDEN = 8 };
typedef struct {
  int32_t x_dim, y_dim;
  int32_t n_hidden, hidden[8];         /* h_dim as the reference's constructor takes it */
  int32_t loss;                        /* VAENMF_MSE_* */
  int32_t max_batch;
  double lr, beta1, beta2, adam_eps;   /* torch.optim.Adam(lr, betas, eps) */
} vaenmf_mask_trainer_config;
int vaenmf_mask_trainer_create(const vaenmf_mask_trainer_config* cfg, vaenmf_mask_trainer** out);
void vaenmf_mask_trainer_destroy(vaenmf_mask_trainer* t);
int vaenmf_mask_trainer_num_tensors(const vaenmf_mask_trainer* t);
int vaenmf_mask_trainer_tensor_shape(const vaenmf_mask_trainer* t, int32_t i, int32_t* rows, int32_t* cols);
int vaenmf_mask_trainer_set_tensor(vaenmf_mask_trainer* t, int32_t which, int32_t i, const float* src, void* stream);
int vaenmf_mask_trainer_get_tensor(const vaenmf_mask_trainer* t, int32_t which, int32_t i, float* dst, void* stream);
int vaenmf_mask_trainer_set_norm(vaenmf_mask_trainer* t, const float* mean, const float* std, float eps);
int64_t vaenmf_mask_trainer_step_count(const vaenmf_mask_trainer* t);
int vaenmf_mask_trainer_set_step_count(vaenmf_mask_trainer* t, int64_t step);
int vaenmf_mask_trainer_step(vaenmf_mask_trainer* t, const float* X, int32_t ldx, const float* Y, int32_t ldy, int64_t NT,
                             const int32_t* idx, int32_t B, double* losses, void* stream);
int vaenmf_mask_trainer_eval(vaenmf_mask_trainer* t, const float* X, int32_t ldx, const float* Y, int32_t ldy, int64_t NT,
                             const int32_t* idx, int32_t B, double* losses, void* stream);

#ifdef __cplusplus
}
#endif
#endif
