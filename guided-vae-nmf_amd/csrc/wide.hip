// MH chain for the wide decoder shapes: z_dim up to 128 and a hidden layer of 256 units (models.py:107-133 is generic;
// scripts/evaluate_M1.py:41-51 lists z_dim = 128 checkpoints with h_dim [256, 128] and [128]).  The reference builds the
// decoder over reversed(h_dim) (models.py:133), so h_dim [256, 128] is the decoder z -> 128 -> 256 -> F; the mirrored
// z -> 256 -> 128 -> F (h_dim [128, 256]) runs as well.  A plan is wide when L > 32 or one of its hidden layers has 256
// units; every other plan keeps the kernels of engine.hip / chain.hip.
//
// One workgroup of four wavefronts per 16-frame wave tile (the tables of vaenmf_bind_batch).  The frames are the MFMA
// column dimension (lane = 16 q + c, frame c), the features of every layer are MFMA rows: wavefront w computes the
// feature tiles w, w + 4, ... of each layer and the activations travel between the wavefronts through LDS in fragment
// order (engine.hip's header describes the order; plan.hip's pack_weights packs the weights in it).  The latents sit in
// Lp = 128 columns, zero beyond L: wavefront w keeps k-step w of the first layer's input (latents 32 w .. 32 w + 31) in
// registers, draws their noise itself and writes their image.
//
// Weights: every fragment is read from global memory (L2) at its use -- 464 KB per evaluation in bf16x3 mode at
// F = 257 with z -> 128 -> 256 -> F, more than the 160 KB of LDS -- so this kernel is bound by the L2 weight stream, not by the MFMA rate
// (DESIGN 3.8).  Only the activation images and the per-frame sums live in LDS.
//
// Contracts (those of mh_chain_kernel, engine.hip): device noise of latent quad j of a frame from
// xs_seed(utt_seed, frame_in_utt, j, call), j = 0..31, the uniform from quad 0's stream after its normals; energy sums
// in fp64 per frame, the four wavefronts' partial sums added in the order 0..3; an utterance's tiles start at its
// first frame, so nothing depends on the batch around it; store rows in plain bin order with exact zeros in the
// padding bins (W3 rows 0, b3 = -200: 2^-200 is 0 in fp32).
#include "common.h"

namespace {

constexpr int WD_LP = 128;         // latent columns of a wide plan
constexpr int WD_MAXT = 10;        // bin tiles per wavefront: 40 tiles at F = 640

struct WideArgs {
  const __bf16 *w1f, *w2f, *w3f;   // [tile][kstep][part][lane][8]: W1 H1/16 x 4, W2 H2/16 x H1/32, W3 Fs/16 x NK3
  const float *b1, *b2, *b3;       // scaled biases; b3 [Fs], padding -200
  int NT1, NT2, NT3;               // feature tiles of layer 1 (8 or 16), of layer 2 (0: one hidden layer, 8 or 16), bin tiles
  int NK1, NK2, NK3;               // k-steps: of layer 1 that hold latents, of layer 2 (H1 / 32), of the output layer (4 or 8)
  int H1, Lz, F, Fs, Kp, NT;
  VnChainCall cc;                  // the call (common.h): its buffers, the store and its layout, the replay draws, counts, step size
  const float* Vb;                 // the plan's fixed noise variance [NT][Fs] or null: Vb = W H
  const int32_t *wt_utt, *wt_n0, *wt_cnt, *frame_off;
  const uint64_t* utt_seed;
};

template <bool SPLIT, bool STORE>
__global__ __launch_bounds__(256) void widechain_kernel(const WideArgs a) {
  constexpr int PARTS = SPLIT ? 2 : 1;
  using store_t = typename std::conditional<SPLIT, float, __bf16>::type;
  // activation images [k-step][part][lane][8 bf16]: the proposal's latents, layers 1 and 2 (up to 256 features each)
  __shared__ __attribute__((aligned(16))) char zimg[4 * PARTS * 1024];
  __shared__ __attribute__((aligned(16))) char act1[8 * PARTS * 1024];
  __shared__ __attribute__((aligned(16))) char act2[8 * PARTS * 1024];
  __shared__ double epart[4][16];            // per wavefront and frame: partial energy
  __shared__ float ppart[4][16];             // partial prior term
  __shared__ float ush[16];                  // the step's uniform per frame

  const VnChainCall& cc = a.cc;
  const int lane = threadIdx.x & 63, q = lane >> 4, c = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned lane16 = lane * 16;
  const int tile = blockIdx.x;
  const int utt = a.wt_utt[tile], n0 = a.wt_n0[tile], cnt = a.wt_cnt[tile];
  // columns behind the tile's last frame shadow it (same inputs, same noise) and store nothing
  const bool fvalid = c < cnt;
  const int nrow = n0 + (fvalid ? c : cnt - 1);
  const float gn = cc.g[nrow];

  // the fragment loaders and the activation store: this kernel's address arithmetic, then common.h's load_frag / store_act_tile
  auto wfrag = [&](const __bf16* base, int t, int nk, int s, bf16x8& hi, bf16x8& lo) {
    load_frag<SPLIT>(reinterpret_cast<const char*>(base) + ((size_t)(t * nk + s) * 2) * 1024 + lane16, hi, lo);
  };
  auto afrag = [&](const char* img, int s, bf16x8& hi, bf16x8& lo) { load_frag<SPLIT>(img + s * PARTS * 1024 + lane16, hi, lo); };
  auto store_act = [&](char* img, int t, const f32x4 acc) { store_act_tile<SPLIT>(img, lane16, t, acc); };

  // ---- per-(bin, frame) constants in accumulator layout: X2 and Vb = W H, padding bins X2 = 0, Vb = 1 (tile_consts4)
  f32x4 x2[WD_MAXT], vb[WD_MAXT];
#pragma unroll
  for (int i = 0; i < WD_MAXT; ++i)
    tile_consts4(w + 4 * i < a.NT3, cc.X2, a.Vb, cc.W, cc.Ht, a.Fs, a.Kp, nrow, utt, 16 * (w + 4 * i) + 4 * q, a.F, x2[i], vb[i]);
  // ---- accumulator init of the hidden layers: b1, or per frame b1 + W1y y_n (M2, vaenmf_layer1_bias); b2
  f32x4 bias1[4], bias2[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int f0 = 16 * (w + 4 * i) + 4 * q;
    bias1[i] = f32x4{0, 0, 0, 0};
    if (w + 4 * i < a.NT1)
      bias1[i] = cc.B1 ? *reinterpret_cast<const f32x4*>(cc.B1 + (size_t)nrow * a.H1 + f0) : *reinterpret_cast<const f32x4*>(a.b1 + f0);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    bias2[i] = w + 4 * i < a.NT2 ? *reinterpret_cast<const f32x4*>(a.b2 + 16 * (w + 4 * i) + 4 * q) : f32x4{0, 0, 0, 0};
  // ---- this lane's latents of its frame, fragment order of k-step w: 32 w + 4 q + (0..3) and 32 w + 16 + 4 q + (0..3)
  const int l0 = 32 * w + 4 * q, l1 = l0 + 16;
  float z[8];
  load_row8(cc.Z + (size_t)nrow * WD_LP, l0, l1, z);
  // ---- noise: latent quads l0 / 4 and l1 / 4 of the frame; quads of padding latents (>= Lz) get none
  const bool on0 = l0 < a.Lz, on1 = l1 < a.Lz;
  Xs128 st0 = {1, 0, 0, 0}, st1 = {1, 0, 0, 0};
  if (cc.rng_mode == VAENMF_RNG_DEVICE) {
    const uint64_t seed = a.utt_seed[utt];
    const uint32_t fr = (uint32_t)(nrow - a.frame_off[utt]);
    if (on0) st0 = xs_seed(seed, fr, (uint32_t)(l0 >> 2), cc.call);
    if (on1) st1 = xs_seed(seed, fr, (uint32_t)(l1 >> 2), cc.call);
  }
  const bool ulane = w == 0 && q == 0;      // quad 0 of the frame: its stream also yields the step's uniform

  // E(z) = sum_f [log Vx + X2 / Vx] of the frame (fp64 sums, as in mh_chain_kernel); also hands every lane the
  // frame's prior term and uniform, which travel with the partial sums
  auto energy = [&](const float (&zz)[8], float pr, float uu, double& E, float& P, float& U, int slot, auto dost) {
    constexpr bool DOST = STORE && decltype(dost)::value;
    {
      bf16x8 hi, lo;
      split8<SPLIT>(zz, hi, lo);
      *reinterpret_cast<bf16x8*>(zimg + w * PARTS * 1024 + lane16) = hi;
      if (SPLIT) *reinterpret_cast<bf16x8*>(zimg + w * PARTS * 1024 + 1024 + lane16) = lo;
    }
    __syncthreads();
    // ---- layer 1
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = w + 4 * i;
      if (t < a.NT1) {
        f32x4 acc = bias1[i];
        for (int s = 0; s < a.NK1; ++s) {
          bf16x8 whi, wlo, ahi, alo;
          wfrag(a.w1f, t, 4, s, whi, wlo);
          afrag(zimg, s, ahi, alo);
          acc = mma3<SPLIT>(whi, wlo, ahi, alo, acc);
        }
        store_act(act1, t, acc);
      }
    }
    __syncthreads();
    // ---- layer 2
    if (a.NT2 > 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = w + 4 * i;
        if (t < a.NT2) {
          f32x4 acc = bias2[i];
          for (int s = 0; s < a.NK2; ++s) {
            bf16x8 whi, wlo, ahi, alo;
            wfrag(a.w2f, t, a.NK2, s, whi, wlo);
            afrag(act1, s, ahi, alo);
            acc = mma3<SPLIT>(whi, wlo, ahi, alo, acc);
          }
          store_act(act2, t, acc);
        }
      }
      __syncthreads();
    }
    // ---- output layer and the frame's energy
    const char* last = a.NT2 > 0 ? act2 : act1;
    char* const vrow = DOST ? reinterpret_cast<char*>(cc.VsS) + ((size_t)nrow * cc.lay.frame + (size_t)slot * cc.lay.row) * sizeof(store_t) : nullptr;
    double e = 0.0;
#pragma unroll
    for (int i = 0; i < WD_MAXT; ++i) {
      const int t = w + 4 * i;
      if (t < a.NT3) {
        f32x4 acc = *reinterpret_cast<const f32x4*>(a.b3 + 16 * t + 4 * q);
        for (int s = 0; s < a.NK3; ++s) {
          bf16x8 whi, wlo, ahi, alo;
          wfrag(a.w3f, t, a.NK3, s, whi, wlo);
          afrag(last, s, ahi, alo);
          acc = mma3<SPLIT>(whi, wlo, ahi, alo, acc);
        }
        f32x4 ev;
        float pl = 0.f, px = 0.f;                       // sum log2 Vx, sum X2 / Vx
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          ev[k] = fast_exp(acc[k]);
          const float vx = gn * ev[k] + vb[i][k];
          pl += fast_log2(vx);
          px += x2[i][k] * fast_rcp(vx);
        }
        if (DOST && fvalid && 16 * t + 4 * q >= (int)cc.lay.row) {      // line-aligned layout: a row ends at bin F-2, bin F-1 has its own block
          if (16 * t + 4 * q == a.F - 1)
            reinterpret_cast<store_t*>(cc.VsS)[cc.lay.xbase + (size_t)nrow * cc.lay.xframe + (size_t)slot * cc.lay.xslot] = (store_t)ev[0];
        } else if (DOST && fvalid) {
          store_t* dst = reinterpret_cast<store_t*>(vrow) + 16 * t + 4 * q;
          if (SPLIT) *reinterpret_cast<f32x4*>(dst) = ev;
          else *reinterpret_cast<bf16x4*>(dst) = bf16x4{(__bf16)ev[0], (__bf16)ev[1], (__bf16)ev[2], (__bf16)ev[3]};
        }
        e += (double)(pl * LN2_F + px);
      }
    }
    e = sum_rows4_d(e);
    pr = sum_rows4(pr);
    if (q == 0) { epart[w][c] = e; ppart[w][c] = pr; }
    if (ulane) ush[c] = uu;
    __syncthreads();
    E = ((epart[0][c] + epart[1][c]) + epart[2][c]) + epart[3][c];
    P = ((ppart[0][c] + ppart[1][c]) + ppart[2][c]) + ppart[3][c];
    U = ush[c];
  };

  double Ecur = 0.0;
  int cur_src = cc.nsamples;
  // the passes of vn_chain_pass (common.h)
  const int n_it = vn_chain_passes<STORE>(cc.nsamples, cc.burnin);
  for (int it = -1; it < n_it; ++it) {
    const VnChainPass ps = vn_chain_pass<STORE>(it, cc.nsamples, cc.burnin);
    const bool re = ps.re, step = ps.step;
    const int m = ps.m, slot = ps.slot;
    // ---- proposal  Z' = Z + sqrt(var) * randn   (mcem.py:407)
    float e8[8] = {0, 0, 0, 0, 0, 0, 0, 0}, uu = 1.f;
    if (step) {
      f32x4 e0 = {0, 0, 0, 0}, e1 = {0, 0, 0, 0};
      if (cc.rng_mode == VAENMF_RNG_DEVICE) {
        if (on0) e0 = normal4(st0);
        if (on1) e1 = normal4(st1);
        if (ulane) uu = uniform01(st0);
      } else {
        const size_t row = (size_t)m * a.NT + nrow;
        if (on0) e0 = *reinterpret_cast<const f32x4*>(cc.eps + row * WD_LP + l0);
        if (on1) e1 = *reinterpret_cast<const f32x4*>(cc.eps + row * WD_LP + l1);
        if (ulane) uu = cc.u[row];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) { e8[k] = e0[k]; e8[4 + k] = e1[k]; }
    }
    const float sd = step ? cc.sd : 0.f;
    float zp[8], pr = 0.f;                              // .5 * sum(Z^2 - Z'^2) follows (mcem.py:417)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      zp[j] = z[j] + sd * e8[j];
      pr += z[j] * z[j] - zp[j] * zp[j];
    }
    double Ep;
    float P, U;
    if (STORE && slot >= 0) energy(zp, pr, uu, Ep, P, U, slot, std::true_type{});
    else energy(zp, pr, uu, Ep, P, U, slot, std::false_type{});
    if (re) continue;                                   // (the state and its energy are untouched)
    const float accp = (float)(Ecur - Ep) + 0.5f * P;   // mcem.py:415-417
    const bool ok = m < 0 || fast_log(U) < accp;        // mcem.py:420
    if (cc.acc_out && m >= 0 && ulane && fvalid) cc.acc_out[(size_t)m * a.NT + nrow] = accp;
    if (ok) {                                           // mcem.py:429-433
#pragma unroll
      for (int j = 0; j < 8; ++j) z[j] = zp[j];
      Ecur = Ep;
      if (STORE && m >= cc.burnin) cur_src = m - cc.burnin;
    }
    if (m >= cc.burnin && fvalid) {
      if (STORE && w == 1 && q == 0) cc.src[(size_t)(m - cc.burnin) * a.NT + nrow] = cur_src;
      if (cc.Zs) store_row8(cc.Zs + ((size_t)nrow * cc.Rcap + (m - cc.burnin)) * WD_LP, l0, l1, z);    // mcem.py:435-437
    }
  }
  if (cc.update_Z && fvalid) store_row8(cc.Z + (size_t)nrow * WD_LP, l0, l1, z);    // self.Z = last draw (mcem.py:466)
}

}  // namespace

int vn_launch_widechain(vaenmf_plan* p, const VnChainCall& cc, hipStream_t st) {
  VN_REQUIRE(p->wide, "vn_launch_widechain: not a wide plan");
  WideArgs a = {};
  a.w1f = p->w1f; a.w2f = p->w2f; a.w3f = p->w3f; a.b1 = p->b1; a.b2 = p->b2; a.b3 = p->b3;
  a.H1 = p->cfg.H1; a.Lz = p->Lz;
  a.NT1 = a.H1 / 16; a.NT2 = p->cfg.H2 / 16; a.NT3 = p->Fs / 16;
  a.NK1 = (p->Lz + 31) / 32; a.NK2 = a.H1 / 32; a.NK3 = (p->one_hidden ? a.H1 : p->cfg.H2) / 32;
  VN_REQUIRE(a.NT3 <= 4 * WD_MAXT && a.NT1 <= 16 && a.NT2 <= 16 && a.NK2 <= 8 && a.NK3 <= 8 && a.NK1 <= 4 && p->Lp == WD_LP,
             "wide chain: shape outside the kernel's tiles");
  a.F = p->cfg.F; a.Fs = p->Fs; a.Kp = p->Kp; a.NT = p->NT;
  a.cc = cc;
  a.Vb = p->Vb_ext;
  a.wt_utt = p->d_wt_utt; a.wt_n0 = p->d_wt_n0; a.wt_cnt = p->d_wt_cnt; a.frame_off = p->d_frame_off;
  a.utt_seed = p->d_utt_seed;
  const bool split = p->cfg.precision == VAENMF_PREC_BF16X3;
  const dim3 grid(p->n_wtiles), blk(256);
  if (split) {
    if (cc.VsS) hipLaunchKernelGGL((widechain_kernel<true, true>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((widechain_kernel<true, false>), grid, blk, 0, st, a);
  } else {
    if (cc.VsS) hipLaunchKernelGGL((widechain_kernel<false, true>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((widechain_kernel<false, false>), grid, blk, 0, st, a);
  }
  VN_CHECK_HIP(hipGetLastError());
  p->last_chain_kernel = 3;
  return 0;
}
