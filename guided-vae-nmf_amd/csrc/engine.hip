// MH-chain and sample-decode kernels: the hot loop of the VAE-NMF reconstruct path.
//
// mh_chain_kernel and decode_kernel evaluate the decoder MLP (python/models/models.py:118-121) on MFMA
// (v_mfma_f32_16x16x32_bf16, fp32 accumulate).  The MLP input rows are the MFMA
// *column* dimension (16 per column group), the features are MFMA rows split over
// the waves of a workgroup, so an accumulator tile of one layer is, after tanh and a
// bf16 (hi,lo) split, directly the B fragment of the next layer (exchanged between
// waves through LDS in fragment order -- no transposes, no shuffles).
//
//   fragment order: k-step s of 32 input features, lane (q = lane>>4, c = lane&15),
//   element j (0..7)  <->  input feature  phi(s,q,j) = 32 s + 16 (j>>2) + 4 q + (j&3)
//   (a 16x16 accumulator tile T holds rows 4q+t of feature tile T in lane group q,
//   so k-step s consumes feature tiles 2s (j<4) and 2s+1 (j>=4)).  The weights are
//   pre-permuted on the host into the same order (plan.hip: pack_weights).
//
// PREC: bf16x3 computes w_hi*a_hi + w_lo*a_hi + w_hi*a_lo (error ~2^-17 per product);
//       bf16 computes w_hi*a_hi only.
//
// What these kernels share with the wide chain (wide.hip) is in common.h: split8, the fragment loader load_frag, the load of
// a latent row.  wide.hip takes more from there (the tanh-split-store of a tile, the row stores, the per-tile constants
// X2 and Vb = W H); here those stay written out, because every form of sharing them changed the instructions of these
// kernels.
#include "common.h"

namespace {

constexpr int TEAM_COLS = 32;      // MLP input rows ("columns") per team and pass: 2 MFMA column groups

struct DecW {                      // decoder weights (device), fragment order [tile][kstep][part][lane][8]
  const __bf16 *w1f, *w2f, *w3f;
  const float *b1, *b2, *b3;
  const float* w3n;                // fp32 row F-1 of the last layer when the odd last bin is off the tiles
  int NT3;                         // feature tiles in the last layer (MFMA path)
  int F;                           // bins
  int Fm;                          // bins on the MFMA path: F-1 when F = 16k+1 (n_fft/2+1: the Nyquist bin would
                                   // cost a whole 16-row tile, a fifth of one wave's work), else F
  int Lz;                          // latent dimension of the model (latents Lz..31 are zero padding: no random-walk noise)
  int one_hidden;                  // decoder with one hidden layer: the output layer reads layer 1's image
};

// A workgroup = NTEAM teams x NW waves.  The NW waves of a team split the output features of
// every layer and share 32 columns (MH chain: 32 frames; decode: 32 samples of one frame);
// the teams work on different columns, share the LDS-resident weights and run in lockstep
// (workgroup barriers), so the two waves a SIMD hosts overlap each other's LDS / L2 latency
// and VALU issue.
//
// LDS carve (one dynamic array; every offset a multiple of 16):
//   w1, w2 (, w3)  weight fragments, PARTS = 2 (hi,lo) in bf16x3 mode, 1 in bf16 mode
//   act[team]      activation image [col group][k-step][part][lane][8 bf16]; layer 1 and
//                  layer 2 images alias each other in bf16x3 mode (one more barrier)
template <int NTEAM, bool SPLIT>
struct LdsMap {
  static constexpr int PARTS = SPLIT ? 2 : 1;
  static constexpr bool ALIAS = SPLIT;                      // act2 aliases act1
  static constexpr int ACT = 2 * NK_H * PARTS * 1024;       // one image (2 col groups)
  static constexpr int ACT_TEAM = ALIAS ? ACT : 2 * ACT;
  static constexpr int W1B = NT_H * 1 * PARTS * 1024;
  static constexpr int W2B = NT_H * NK_H * PARTS * 1024;
  static constexpr int act = 0;
  static constexpr int w1 = act + NTEAM * ACT_TEAM;
  static constexpr int w2 = w1 + W1B;
  static constexpr int b2 = w2 + W2B;              // float[HID]
  static constexpr int b3 = b2 + HID * 4;          // float[640]
  static constexpr int nyq = b3 + 640 * 4;         // float[NTEAM][8 waves][2 col groups][16]: partial logits of the odd last bin
  static constexpr int common_end = nyq + NTEAM * 8 * 2 * 16 * 4;
  static __host__ __device__ constexpr int w3_bytes(int NT3) { return NT3 * NK_H * PARTS * 1024; }
};

// copy fragment blocks global -> LDS (PARTS==1 keeps the hi block only)
template <int PARTS>
__device__ __forceinline__ void stage_weights(char* dst, const __bf16* src, int nblocks /* tile*kstep */) {
  const int nthr = blockDim.x;
  for (int e = threadIdx.x; e < nblocks * PARTS * 64; e += nthr) {       // 16-byte chunks
    const int chunk = e & 63, blk = e >> 6;
    const int b = blk / PARTS, part = blk - b * PARTS;
    const f32x4 v = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(src) + ((size_t)(b * 2 + part) * 64 + chunk) * 16);
    *reinterpret_cast<f32x4*>(dst + (size_t)e * 16) = v;
  }
}

template <bool SPLIT>
__device__ __forceinline__ f32x4 mma3_flip(const bf16x8 ahi, const bf16x8 alo, const bf16x8 whi, const bf16x8 wlo, f32x4 acc) {
  // activations are the A operand (rows = samples), weights the B operand (cols = features)
  if (SPLIT) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi, wlo, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alo, whi, acc, 0, 0, 0);
  }
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi, whi, acc, 0, 0, 0);
}

// Everything a wave needs to run the decoder: LDS pointers + its (uniform) team / wave index.
template <int NW, int NTEAM, int MT, bool SPLIT, bool W3LDS>
struct Dec {
  using M = LdsMap<NTEAM, SPLIT>;
  static constexpr int TPW = NT_H / NW;
  char* lds;
  char* act1;           // this team's layer-1 image
  char* act2;           // this team's layer-2 image (== act1 when aliased)
  const char* w3g;      // global W3 fragments of this wave's first tile (uniform pointer)   [!W3LDS]
  const char* w3l;      // LDS W3 fragments                                                  [W3LDS]
  int w, team, NT3;
  int one_hidden;       // decoder with ONE hidden layer (models.py:107-121, h_dim = [128]): act2 == act1, layer 2 skipped
  unsigned lane16;
  bool nyq;             // the odd last bin is computed beside the tiles
  f32x4 wn[NT_H / NW];  // its weights for this lane's hidden features (rows 4q+t of this wave's layer-2 tiles)
  float* nyqbuf;        // this team's [wave][col group][16] partial sums in LDS

  // Teams run in lockstep through workgroup barriers.  (A per-team LDS-counter barrier was tried:
  // decoupling the teams did not pay -- mh_chain 0.62 -> 0.68 ms per launch -- so it was dropped.)
  __device__ __forceinline__ void team_sync() const { __syncthreads(); }

  // MT == 4 instantiations are only launched when every wave owns exactly 4 bin tiles (NT3 == 4 NW:
  // F = 257 with 4 waves, F = 513 with 8), so their tile loops carry no validity checks
  __device__ __forceinline__ bool tile_ok(int i) const { return MT == 4 || w + NW * i < NT3; }

  static __device__ __forceinline__ int act_off(int cg, int s) { return (cg * NK_H + s) * M::PARTS * 1024; }

  // the fragment loaders: the address arithmetic of each block, then load_frag (common.h)
  __device__ __forceinline__ void lds_w(int base, int tile, int nk, int s, bf16x8& hi, bf16x8& lo) const {
    load_frag<SPLIT>(lds + base + ((tile * nk + s) * M::PARTS) * 1024 + lane16, hi, lo);
  }
  __device__ __forceinline__ void w3_frag(int i, int s, bf16x8& hi, bf16x8& lo) const {
    if (W3LDS) load_frag<SPLIT>(w3l + (((w + NW * i) * NK_H + s) * M::PARTS) * 1024 + lane16, hi, lo);
    else load_frag<SPLIT>(w3g + (size_t)((i * NW * NK_H + s) * 2) * 1024 + lane16, hi, lo);
  }
  __device__ __forceinline__ void act_frag(const char* img, int cg, int s, bf16x8& hi, bf16x8& lo) const {
    load_frag<SPLIT>(img + act_off(cg, s) + lane16, hi, lo);
  }
  // split + store one tile of activations (feature tile `tile`, already tanh'ed) into an LDS image
  __device__ __forceinline__ void store_h(char* img, int cg, int tile, const f32x4 h) const {
    const int s = tile >> 1, e = tile & 1;
    bf16x4 hi, lo;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      __bf16 x = (__bf16)h[t];
      hi[t] = x;
      lo[t] = (__bf16)(h[t] - (float)x);
    }
    *reinterpret_cast<bf16x4*>(img + act_off(cg, s) + lane16 + e * 8) = hi;
    if (SPLIT) *reinterpret_cast<bf16x4*>(img + act_off(cg, s) + 1024 + lane16 + e * 8) = lo;
  }
  static __device__ __forceinline__ f32x4 tanh4(const f32x4 a) {
    f32x4 h;
#pragma unroll
    for (int t = 0; t < 4; ++t) h[t] = fast_tanh(a[t]);
    return h;
  }
  __device__ __forceinline__ void store_act(char* img, int cg, int tile, f32x4 acc) const { store_h(img, cg, tile, tanh4(acc)); }
  // logit of the odd last bin for column (cg, lane&15): sum of the waves' partial dot products + bias
  __device__ __forceinline__ float nyq_logit(int cg, float bias) const {
    float a = bias;
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) a += nyqbuf[(ww * 2 + cg) * 16 + ((lane16 >> 4) & 15)];
    return a;
  }

  // Hidden layers 1 and 2 for this team's two column groups.  zhi/zlo: layer-1 B fragments
  // (latent rows); bias1[ti][cg]: accumulator init of layer 1.  Leaves tanh(layer 2) in act2.
  // `between` runs after the first barrier (all waves have consumed the previous step's noise).
  template <typename F>
  __device__ __forceinline__ void hidden(const bf16x8 (&zhi)[2], const bf16x8 (&zlo)[2], const f32x4 (&bias1)[TPW][2], F between) const {
    if (one_hidden) {       // (wave-uniform) layer 1 is the last hidden layer: its image is the output layer's input
      float pn[2] = {0.f, 0.f};
#pragma unroll
      for (int ti = 0; ti < TPW; ++ti) {
        const int tile = w + NW * ti;
        bf16x8 whi, wlo;
        lds_w(M::w1, tile, 1, 0, whi, wlo);
#pragma unroll
        for (int cg = 0; cg < 2; ++cg) {
          const f32x4 h = tanh4(mma3<SPLIT>(whi, wlo, zhi[cg], zlo[cg], bias1[ti][cg]));
          store_h(act1, cg, tile, h);
          pn[cg] += h[0] * wn[ti][0] + h[1] * wn[ti][1] + h[2] * wn[ti][2] + h[3] * wn[ti][3];
        }
      }
      if (nyq) {
#pragma unroll
        for (int cg = 0; cg < 2; ++cg) {
          const float v = sum_rows4(pn[cg]);
          if ((lane16 >> 8) == 0) nyqbuf[(w * 2 + cg) * 16 + ((lane16 >> 4) & 15)] = v;
        }
      }
      team_sync();
      between();
      return;
    }
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti) {
      const int tile = w + NW * ti;
      bf16x8 whi, wlo;
      lds_w(M::w1, tile, 1, 0, whi, wlo);
#pragma unroll
      for (int cg = 0; cg < 2; ++cg) store_act(act1, cg, tile, mma3<SPLIT>(whi, wlo, zhi[cg], zlo[cg], bias1[ti][cg]));
    }
    team_sync();
    between();
    f32x4 acc2[TPW][2];
    const float* b2 = reinterpret_cast<const float*>(lds + M::b2);
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti) {
      const f32x4 bv = *reinterpret_cast<const f32x4*>(b2 + 16 * (w + NW * ti) + (lane16 >> 8) * 4);   // 4*q
      acc2[ti][0] = bv; acc2[ti][1] = bv;
    }
#pragma unroll
    for (int s = 0; s < NK_H; ++s) {
      bf16x8 ahi[2], alo[2];
      act_frag(act1, 0, s, ahi[0], alo[0]);
      act_frag(act1, 1, s, ahi[1], alo[1]);
#pragma unroll
      for (int ti = 0; ti < TPW; ++ti) {
        bf16x8 whi, wlo;
        lds_w(M::w2, w + NW * ti, NK_H, s, whi, wlo);
#pragma unroll
        for (int cg = 0; cg < 2; ++cg) acc2[ti][cg] = mma3<SPLIT>(whi, wlo, ahi[cg], alo[cg], acc2[ti][cg]);
      }
    }
    if (M::ALIAS) team_sync();      // every wave is done reading the layer-1 image
    float pn[2] = {0.f, 0.f};
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
      for (int cg = 0; cg < 2; ++cg) {
        const f32x4 h = tanh4(acc2[ti][cg]);
        store_h(act2, cg, w + NW * ti, h);
        pn[cg] += h[0] * wn[ti][0] + h[1] * wn[ti][1] + h[2] * wn[ti][2] + h[3] * wn[ti][3];
      }
    if (nyq) {           // fp32 partial dot of the odd last bin over this wave's hidden features
#pragma unroll
      for (int cg = 0; cg < 2; ++cg) {
        const float v = sum_rows4(pn[cg]);
        if ((lane16 >> 8) == 0) nyqbuf[(w * 2 + cg) * 16 + ((lane16 >> 4) & 15)] = v;
      }
    }
    team_sync();
  }

  // Output layer of the chain, bins x frames (acc rows = bins 16 tile + 4q + t, columns = the frames of a column group),
  // tile-major: the activation fragments of all k-steps are read once, then each bin tile is finished (MFMAs over the
  // k-steps) and handed to `epi(i, acc0, acc1)` before the next one starts, so the VALU epilogue of tile i can run under
  // the MFMAs of tile i+1 (same wave, independent instructions).
  template <typename BIAS, typename EPI>
  __device__ __forceinline__ void out_bins_by_frames(BIAS bias, EPI epi) const {
    bf16x8 ahi[NK_H][2], alo[NK_H][2];
#pragma unroll
    for (int s = 0; s < NK_H; ++s) {
      act_frag(act2, 0, s, ahi[s][0], alo[s][0]);
      act_frag(act2, 1, s, ahi[s][1], alo[s][1]);
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      if (tile_ok(i)) {
        f32x4 acc[2];
        acc[0] = bias(i);
        acc[1] = acc[0];
#pragma unroll
        for (int s = 0; s < NK_H; ++s) {
          bf16x8 whi, wlo;
          w3_frag(i, s, whi, wlo);
#pragma unroll
          for (int cg = 0; cg < 2; ++cg) acc[cg] = mma3<SPLIT>(whi, wlo, ahi[s][cg], alo[s][cg], acc[cg]);
        }
        epi(i, acc[0], acc[1]);
      }
    }
  }

  // Output layer of decoding, samples x bins (acc[i][cg] rows = the samples 4q + t of a column group, column = bin
  // 16 tile + c), k-step-major: the activations are the A operand here (mma3_flip).
  __device__ __forceinline__ void out_samples_by_bins(f32x4 (&acc)[MT][2]) const {
#pragma unroll
    for (int s = 0; s < NK_H; ++s) {
      bf16x8 ahi[2], alo[2];
      act_frag(act2, 0, s, ahi[0], alo[0]);
      act_frag(act2, 1, s, ahi[1], alo[1]);
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        if (tile_ok(i)) {   // wave-uniform (w is an SGPR value)
          bf16x8 whi, wlo;
          w3_frag(i, s, whi, wlo);
#pragma unroll
          for (int cg = 0; cg < 2; ++cg) acc[i][cg] = mma3_flip<SPLIT>(ahi[cg], alo[cg], whi, wlo, acc[i][cg]);
        }
      }
    }
  }
};

// workgroup prologue of mh_chain_kernel and decode_kernel: stage W1/W2 (and W3 when it fits), b2, b3 into LDS
template <int NW, int NTEAM, int MT, bool SPLIT, bool W3LDS>
__device__ __forceinline__ Dec<NW, NTEAM, MT, SPLIT, W3LDS> dec_setup(char* smem, const DecW& dw, int w3_lds_off, int Fs) {
  using M = LdsMap<NTEAM, SPLIT>;
  Dec<NW, NTEAM, MT, SPLIT, W3LDS> d;
  d.lds = smem;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  d.team = wid / NW;
  // logical wave index, rotated per team: waves w and w+NW share a SIMD, so the wave with one bin tile
  // more than the others sits on a different SIMD in each team
  d.w = (wid - d.team * NW + (NW / 2) * d.team) % NW;
  d.lane16 = (threadIdx.x & 63) * 16;
  d.NT3 = dw.NT3;
  d.act1 = smem + M::act + d.team * M::ACT_TEAM;
  d.one_hidden = dw.one_hidden;
  d.act2 = (M::ALIAS || dw.one_hidden) ? d.act1 : d.act1 + M::ACT;
  d.w3g = reinterpret_cast<const char*>(dw.w3f) + (size_t)d.w * NK_H * 2 * 1024;
  d.w3l = smem + (W3LDS ? w3_lds_off : 0);
  d.nyq = dw.Fm != dw.F;
  d.nyqbuf = reinterpret_cast<float*>(smem + M::nyq) + d.team * 8 * 2 * 16;
#pragma unroll
  for (int ti = 0; ti < NT_H / NW; ++ti)
    d.wn[ti] = d.nyq ? *reinterpret_cast<const f32x4*>(dw.w3n + 16 * (d.w + NW * ti) + 4 * ((threadIdx.x & 63) >> 4)) : f32x4{0, 0, 0, 0};
  stage_weights<M::PARTS>(smem + M::w1, dw.w1f, NT_H);
  stage_weights<M::PARTS>(smem + M::w2, dw.w2f, NT_H * NK_H);
  if (W3LDS) stage_weights<M::PARTS>(smem + w3_lds_off, dw.w3f, dw.NT3 * NK_H);
  float* b2 = reinterpret_cast<float*>(smem + M::b2);
  float* b3 = reinterpret_cast<float*>(smem + M::b3);
  for (int i = threadIdx.x; i < HID; i += blockDim.x) b2[i] = dw.b2[i];
  for (int i = threadIdx.x; i < Fs; i += blockDim.x) b3[i] = dw.b3[i];
  return d;
}

__device__ __forceinline__ double shfl_xor_d(double v, int m) { return __shfl_xor(v, m, 64); }

// Diagnostic builds only (-DVN_STAMP): per-phase cycle sums of workgroup 0 / wave 0 into a debug buffer
// that nothing else reads.  The shipped library never executes a stamp.
#ifdef VN_STAMP
__device__ long long* g_stamp_buf = nullptr;
__device__ long long g_stamp_store[64];
#define VN_STAMP_DECL long long _t_prev = (long long)__builtin_amdgcn_s_memtime(); const bool _st_on = blockIdx.x == 0 && threadIdx.x == 0;
#define VN_STAMP_AT(slot) do { long long _t = (long long)__builtin_amdgcn_s_memtime(); if (_st_on) { g_stamp_store[slot] += _t - _t_prev; g_stamp_store[32 + slot] += 1; } _t_prev = _t; } while (0)
#else
#define VN_STAMP_DECL
#define VN_STAMP_AT(slot)
#endif

// ============================================================================
// MH chain (mcem.py:371-441 / :218-294)
// ============================================================================
struct ChainArgs {
  DecW dw;
  const float *X2, *W, *Ht, *g, *B1;
  const float* Vb;           // external noise variance [NT][Fs] (the *_noNMF variants, mcem.py:493-760) or null: Vb = W H
  float *Z, *Zs, *acc_out;
  void* VsS;                 // sample-variance store (float in bf16x3 mode, bf16 in bf16 mode), laid out as `lay`, or null
  VnStoreLayout lay;         // (common.h)
  int32_t* src;              // [Rs][NT] (sample-major): slot of VsS that holds the variances of sample r of frame n
  int Rs;                    // slots per frame: nsamples + 1
  const int32_t *tile_utt, *tile_n0, *tile_cnt, *frame_off;
  const uint64_t* utt_seed;
  const float *eps, *u;      // replay buffers or null
  int Fs, Kp, NT, Rcap, nsamples, burnin, rng_mode, update_Z;
  int w3_lds_off;            // LDS offset of the W3 fragments, or -1 (streamed from L2)
  uint32_t call;
  float sd;                  // sqrt(var_RW)
};

// chain-specific LDS after LdsMap::common_end, one per team
struct ChainX {
  float eps[TEAM_COLS][LAT];
  float u[TEAM_COLS];
  double epart[2][8][TEAM_COLS];
};

template <int NW, int NTEAM, int MT, bool SPLIT, bool W3LDS, bool STORE>
__global__ __launch_bounds__(NW * NTEAM * 64) void mh_chain_kernel(const ChainArgs a) {
  constexpr int MAXT = MT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using M = LdsMap<NTEAM, SPLIT>;
  constexpr int TPW = NT_H / NW;
  const DecW& dw = a.dw;
  const Dec<NW, NTEAM, MT, SPLIT, W3LDS> d = dec_setup<NW, NTEAM, MT, SPLIT, W3LDS>(smem, dw, a.w3_lds_off, a.Fs);
  ChainX& L = reinterpret_cast<ChainX*>(smem + M::common_end)[d.team];
  const int lane = threadIdx.x & 63, w = d.w, q = lane >> 4, c = lane & 15;
  const int tile = blockIdx.x;
  const int utt = a.tile_utt[tile];
  const int cnt_all = a.tile_cnt[tile];                                 // <= 32*NTEAM frames, one utterance
  int cnt = cnt_all - TEAM_COLS * d.team;                               // this team's share
  cnt = cnt < 0 ? 0 : (cnt > TEAM_COLS ? TEAM_COLS : cnt);
  const bool team_on = cnt > 0;
  const int n0 = a.tile_n0[tile] + (team_on ? TEAM_COLS * d.team : 0);  // idle team shadows team 0 (no stores)
  if (!team_on) cnt = cnt_all < TEAM_COLS ? cnt_all : TEAM_COLS;

  // ---- frames of this lane (one per column group)
  int nrow[2];
  bool fvalid[2];
  float gn[2];
#pragma unroll
  for (int fg = 0; fg < 2; ++fg) {
    const int j = 16 * fg + c;
    fvalid[fg] = team_on && j < cnt;
    nrow[fg] = n0 + (j < cnt ? j : cnt - 1);
    gn[fg] = a.g[nrow[fg]];
  }
  // ---- per-(bin,frame) constants in accumulator layout: X2 and Vb = W H (mcem.py:81-82).
  // Padding bins get X2 = 0, Vb = 1 and (through b3 = -100, W3 = 0) Vs = 0: their term is exactly 0.
  f32x4 x2[MAXT][2], vb[MAXT][2];
#pragma unroll
  for (int i = 0; i < MAXT; ++i) {
    const int t16 = w + NW * i;
    const int f0 = 16 * t16 + 4 * q;
    const bool tv = d.tile_ok(i);
#pragma unroll
    for (int fg = 0; fg < 2; ++fg) {
      f32x4 xv = tv ? *reinterpret_cast<const f32x4*>(a.X2 + (size_t)nrow[fg] * a.Fs + f0) : f32x4{0, 0, 0, 0};
      f32x4 v = {0, 0, 0, 0};
      if (tv && a.Vb) {
        v = *reinterpret_cast<const f32x4*>(a.Vb + (size_t)nrow[fg] * a.Fs + f0);
      } else if (tv) {
        for (int k = 0; k < a.Kp; k += 4) {
          const f32x4 h = *reinterpret_cast<const f32x4*>(a.Ht + (size_t)nrow[fg] * a.Kp + k);
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const f32x4 wr = *reinterpret_cast<const f32x4*>(a.W + ((size_t)utt * a.Fs + f0 + t) * a.Kp + k);
            v[t] += wr[0] * h[0] + wr[1] * h[1] + wr[2] * h[2] + wr[3] * h[3];
          }
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (f0 + t >= dw.Fm) { xv[t] = 0.f; v[t] = 1.f; }
      x2[i][fg] = xv;
      vb[i][fg] = v;
    }
  }
  // ---- the odd last bin (F = 16k+1), column-on-lane: constants of frame (fg, c)
  float x2n[2] = {0.f, 0.f}, vbn[2] = {1.f, 1.f};
  if (d.nyq) {
#pragma unroll
    for (int fg = 0; fg < 2; ++fg) {
      x2n[fg] = a.X2[(size_t)nrow[fg] * a.Fs + dw.F - 1];
      float v = 0.f;
      if (a.Vb) v = a.Vb[(size_t)nrow[fg] * a.Fs + dw.F - 1];
      else
        for (int k = 0; k < a.Kp; ++k) v += a.W[((size_t)utt * a.Fs + dw.F - 1) * a.Kp + k] * a.Ht[(size_t)nrow[fg] * a.Kp + k];
      vbn[fg] = v;
    }
  }
  // ---- layer-1 accumulator init: b1, or per frame b1 + W1y y_n (M2, folded by vaenmf_layer1_bias)
  f32x4 bias1[TPW][2];
#pragma unroll
  for (int ti = 0; ti < TPW; ++ti) {
    const int f0 = 16 * (w + NW * ti) + 4 * q;
#pragma unroll
    for (int fg = 0; fg < 2; ++fg)
      bias1[ti][fg] = a.B1 ? *reinterpret_cast<const f32x4*>(a.B1 + (size_t)nrow[fg] * HID + f0)
                           : *reinterpret_cast<const f32x4*>(dw.b1 + f0);
  }
  // ---- current latent state, fragment order: latents 4q..4q+3 and 16+4q..16+4q+3
  float z[2][8];
#pragma unroll
  for (int fg = 0; fg < 2; ++fg) load_row8(a.Z + (size_t)nrow[fg] * LAT, 4 * q, 16 + 4 * q, z[fg]);
  // ---- sample-variance store (STORE): the decoded variances Vs = exp(decoder(Z')) of every post-burn-in
  // proposal go to HBM (slot r of the frame for step burnin + r) so that the M-step streams them instead of
  // decoding the samples again; slot R holds the state the chain is in when the burn-in ends (one extra
  // evaluation pass; the initial state itself when there is no burn-in).  src[r][frame] names the slot of the
  // state the chain is in after post-burn-in step r (mcem.py:429-437).
  // The rows are float in bf16x3 mode and bf16 in bf16 mode (half the HBM traffic; the decoder's own bf16 products
  // already carry errors of that size, and each stored value enters the M-step inside a sum over the samples).
  using store_t = typename std::conditional<SPLIT, float, __bf16>::type;
  // (addresses: uniform base + 32-bit element offset of this lane's first bin in slot 0 of its frame -- the host
  // keeps the store below 4 GB -- so the store costs two VGPRs of state, not eight)
  // Lanes without a frame write to a spare frame block behind the last one: the tile stores then need no
  // per-lane predicate (an exec-masked store after every bin tile splits the epilogue into small basic blocks
  // and costs the MFMA / VALU interleave).
  uint32_t voff[2] = {0u, 0u};
  int cur_src[2] = {a.nsamples, a.nsamples};
  if (STORE) {
#pragma unroll
    for (int fg = 0; fg < 2; ++fg)      // BYTE offset (the host keeps the store below 4 GB)
      voff[fg] = ((uint32_t)(fvalid[fg] ? nrow[fg] : a.NT) * a.lay.frame + 4u * q) * (uint32_t)sizeof(store_t);
  }
  // ---- noise streams: thread of the team <-> (frame of the team, latent quad); 256 streams
  const int sid = threadIdx.x - d.team * NW * 64, sfr = sid >> 3, squad = sid & 7;
  const bool srng = sid < TEAM_COLS * 8;
  const bool sval = srng && team_on && sfr < cnt;
  Xs128 st;
  if (sval && a.rng_mode == VAENMF_RNG_DEVICE)
    st = xs_seed(a.utt_seed[utt], (uint32_t)(n0 - a.frame_off[utt] + sfr), (uint32_t)squad, a.call);
  auto draw = [&](int step) {   // noise of MH step `step` -> LDS (single buffer, see Dec::hidden)
    if (!srng) return;
    f32x4 e = {0, 0, 0, 0};
    float uu = 0.5f;
    if (sval) {
      if (a.rng_mode == VAENMF_RNG_DEVICE) {
        e = normal4(st);
        if (squad == 0) uu = uniform01(st);
      } else {
        const size_t row = (size_t)step * a.NT + n0 + sfr;
        e = *reinterpret_cast<const f32x4*>(a.eps + row * LAT + 4 * squad);
        if (squad == 0) uu = a.u[row];
        // retire the replay loads here: otherwise the compiler waits for vmcnt(0) where the two generator paths
        // join, and in the on-device path that wait drains the variance stores of the previous step
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0), gfx9 encoding
      }
    }
    if (4 * squad >= a.dw.Lz) e = f32x4{0, 0, 0, 0};      // padding of a 16-dimensional latent space: no random walk
    *reinterpret_cast<f32x4*>(&L.eps[sfr][4 * squad]) = e;
    if (squad == 0) L.u[sfr] = uu;
  };

  int ecount = 0;
  const float* b3l = reinterpret_cast<const float*>(smem + M::b3);
  const int S = a.nsamples + a.burnin;
  // E(z) = sum_f [log Vx + X2/Vx] per frame (fp64 accumulation: the reference sums the
  // per-bin DIFFERENCES of two states, mcem.py:415-416; summing each state separately
  // needs the extra bits to keep the same absolute accuracy).
  // next_step: the MH step whose noise is drawn during this evaluation (>= S: none); slot: store slot (DOST)
  auto energy = [&](const float (&zz)[2][8], double (&E)[2], int next_step, int slot, auto dost) {
    constexpr bool DOST = STORE && decltype(dost)::value;
    // uniform base (+ slot, SGPR) + 32-bit per-lane byte offset + the tile's constant: no 64-bit VALU address math
    char* const vbase = reinterpret_cast<char*>(a.VsS) + (DOST ? (size_t)slot * a.lay.row * sizeof(store_t) : 0);
    bf16x8 zhi[2], zlo[2];
    split8<SPLIT>(zz[0], zhi[0], zlo[0]);
    split8<SPLIT>(zz[1], zhi[1], zlo[1]);
    d.hidden(zhi, zlo, bias1, [&]() { if (next_step < S) draw(next_step); });
    double e[2] = {0.0, 0.0};
    d.out_bins_by_frames(
        [&](int i) { return *reinterpret_cast<const f32x4*>(b3l + 16 * (w + NW * i) + 4 * q); },
        [&](int i, const f32x4 acc0, const f32x4 acc1) {
#pragma unroll
          for (int fg = 0; fg < 2; ++fg) {
            const f32x4 acc = fg == 0 ? acc0 : acc1;
            // two bins at a time: log Vx0 + log Vx1 = log(Vx0 Vx1) and X0/Vx0 + X1/Vx1 = (X0 Vx1 + X1 Vx0)/(Vx0 Vx1)
            // share one product, one log and one reciprocal (variances outside 1e-19..1e19 have no fp32 square
            // in the M-step either)
            float pl = 0.f, px = 0.f;                       // sum log2 Vx, sum X2 / Vx
            f32x4 ev;
#pragma unroll
            for (int t = 0; t < 4; ++t) ev[t] = fast_exp(acc[t]);
#pragma unroll
            for (int t = 0; t < 4; t += 2) {
              const float v0 = gn[fg] * ev[t] + vb[i][fg][t];
              const float v1 = gn[fg] * ev[t + 1] + vb[i][fg][t + 1];
              const float pp = v0 * v1;
              pl += fast_log2(pp);
              px += (x2[i][fg][t] * v1 + x2[i][fg][t + 1] * v0) * fast_rcp(pp);
            }
            if (DOST) {
              // SGPR base + 32-bit VGPR offset form of the store, written out: the compiler builds a 64-bit VGPR
              // address per store otherwise (3 VALU instructions each, 8 stores per step)
              const char* tb = vbase + 16 * (w + NW * i) * sizeof(store_t);
              if (SPLIT) {
                // (a store of more than 8 bytes needs 2 wait states before its data registers are overwritten)
                asm volatile("global_store_dwordx4 %0, %1, %2\n\ts_nop 1" :: "v"(voff[fg]), "v"(ev), "s"(tb) : "memory");
              } else {
                const bf16x4 pk = bf16x4{(__bf16)ev[0], (__bf16)ev[1], (__bf16)ev[2], (__bf16)ev[3]};
                asm volatile("global_store_dwordx2 %0, %1, %2" :: "v"(voff[fg]), "v"(pk), "s"(tb) : "memory");
              }
            }
            e[fg] += (double)(pl * LN2_F + px);
          }
        });
    if (d.nyq) {
      const float bn = b3l[dw.F - 1];
#pragma unroll
      for (int fg = 0; fg < 2; ++fg) {
        const float vs = fast_exp(d.nyq_logit(fg, bn));
        const float vx = gn[fg] * vs + vbn[fg];
        const float term = fast_log(vx) + x2n[fg] * fast_rcp(vx);
        e[fg] += (w == 0 && q == 0) ? (double)term : 0.0;        // counted once per frame
        if (DOST && w == 2 && q == 0 && a.lay.aligned) {
          // line-aligned layout: the bin goes to the frame's block of odd bins (this kernel only has to be correct there: the
          // wave-private chains, which run these shapes, write a frame's block once, in 16-byte pieces)
          reinterpret_cast<store_t*>(a.VsS)[a.lay.xbase + (size_t)(fvalid[fg] ? nrow[fg] : a.NT) * a.lay.xframe + (size_t)slot * a.lay.xslot] = (store_t)vs;
        } else
        if (DOST && w == 2 && q == 0) {      // (the per-step bookkeeping stores are spread over the waves of the team)
          // the whole 16-bin tail of the row (the bin and its zero padding) in full 32-byte sectors: a lone 2- or
          // 4-byte store per frame and step is a read-modify-write in the memory system (measured: 5 % of the launch)
          store_t* dst = reinterpret_cast<store_t*>(vbase + (size_t)dw.Fm * sizeof(store_t) + voff[fg]);
          if (SPLIT) {
            *reinterpret_cast<f32x4*>(dst) = f32x4{vs, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 1; j < 4; ++j) *reinterpret_cast<f32x4*>(dst + 4 * j) = f32x4{0.f, 0.f, 0.f, 0.f};
          } else {
            bf16x8 t8;
#pragma unroll
            for (int j = 0; j < 8; ++j) t8[j] = (__bf16)0.f;
            bf16x8 h8 = t8;
            h8[0] = (__bf16)vs;
            *reinterpret_cast<bf16x8*>(dst) = h8;
            *reinterpret_cast<bf16x8*>(dst + 8) = t8;
          }
        }
      }
    }
    const int par = ecount & 1;
    ++ecount;
#pragma unroll
    for (int fg = 0; fg < 2; ++fg) {
      e[fg] = sum_rows4_d(e[fg]);
      if (q == 0) L.epart[par][w][16 * fg + c] = e[fg];
    }
    d.team_sync();
#pragma unroll
    for (int fg = 0; fg < 2; ++fg) {
      double s = 0.0;
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) s += L.epart[par][ww][16 * fg + c];
      E[fg] = s;
    }
  };

  __syncthreads();                                    // staged weights and biases
  // retire the prologue's loads here: a counted vmcnt wait for them placed inside the loop would, on every
  // later iteration, wait for the previous step's stores instead (vmcnt counts loads and stores in order)
  __builtin_amdgcn_s_waitcnt(0x0F70);                 // vmcnt(0), gfx9 encoding
  double Ecur[2] = {0.0, 0.0};
  // the passes of vn_chain_pass (common.h): the initial state, Vs_t = decoder(Z_t), then the MH steps
  const int n_it = vn_chain_passes<STORE>(a.nsamples, a.burnin);
  for (int it = -1; it < n_it; ++it) {
    const VnChainPass ps = vn_chain_pass<STORE>(it, a.nsamples, a.burnin);
    const bool re = ps.re;
    const int m = ps.m, slot = ps.slot;
    // ---- proposal  Z' = Z + sqrt(var) * randn   (mcem.py:407)
    float zp[2][8];
    float e8[2][8];
    const float sd = (m < 0 || re) ? 0.f : a.sd;
#pragma unroll
    for (int fg = 0; fg < 2; ++fg) {
      f32x4 e0 = {0, 0, 0, 0}, e1 = {0, 0, 0, 0};
      if (m >= 0 && !re) {
        e0 = *reinterpret_cast<const f32x4*>(&L.eps[16 * fg + c][4 * q]);
        e1 = *reinterpret_cast<const f32x4*>(&L.eps[16 * fg + c][16 + 4 * q]);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        e8[fg][t] = e0[t]; e8[fg][4 + t] = e1[t];
        zp[fg][t] = z[fg][t] + sd * e0[t];
        zp[fg][4 + t] = z[fg][4 + t] + sd * e1[t];
      }
    }
    const float uu0 = (m >= 0 && !re) ? L.u[c] : 1.f, uu1 = (m >= 0 && !re) ? L.u[16 + c] : 1.f;
    double Ep[2];
    // mcem.py:410-412 (draws the next step's noise inside); two copies of the evaluation, with and without stores
    if (STORE && slot >= 0) energy(zp, Ep, re ? S : m + 1, slot, std::true_type{});
    else energy(zp, Ep, re ? S : m + 1, slot, std::false_type{});
    if (re) continue;                                 // (the state, its energy and the pending noise are untouched)
#pragma unroll
    for (int fg = 0; fg < 2; ++fg) {
      float pr = 0.f;                                 // .5*sum(Z^2 - Z'^2)  (mcem.py:417)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float zn = z[fg][j] + sd * e8[fg][j];
        pr += z[fg][j] * z[fg][j] - zn * zn;
      }
      pr = sum_rows4(pr);
      const float accp = (float)(Ecur[fg] - Ep[fg]) + 0.5f * pr;
      const float uu = fg == 0 ? uu0 : uu1;
      const bool ok = m < 0 || fast_log(uu) < accp;   // mcem.py:420
      if (a.acc_out && m >= 0 && w == 3 && q == 0 && fvalid[fg]) a.acc_out[(size_t)m * a.NT + nrow[fg]] = accp;
      if (ok) {                                       // mcem.py:429-433
#pragma unroll
        for (int j = 0; j < 8; ++j) z[fg][j] = z[fg][j] + sd * e8[fg][j];
        Ecur[fg] = Ep[fg];
        if (STORE && m >= a.burnin) cur_src[fg] = m - a.burnin;
      }
      if (STORE && m >= a.burnin && w == 1 && q == 0 && fvalid[fg]) a.src[(size_t)(m - a.burnin) * a.NT + nrow[fg]] = cur_src[fg];   // [r][n]: the 16 frames of a column group fill one line
      if (m >= a.burnin && w == 0 && fvalid[fg]) {    // mcem.py:435-437
        float* dst = a.Zs + ((size_t)nrow[fg] * a.Rcap + (m - a.burnin)) * LAT;
        *reinterpret_cast<f32x4*>(dst + 4 * q) = f32x4{z[fg][0], z[fg][1], z[fg][2], z[fg][3]};
        *reinterpret_cast<f32x4*>(dst + 16 + 4 * q) = f32x4{z[fg][4], z[fg][5], z[fg][6], z[fg][7]};
      }
    }
  }
  if (w == 0 && a.update_Z) {                         // self.Z = last draw (mcem.py:466)
#pragma unroll
    for (int fg = 0; fg < 2; ++fg)
      if (fvalid[fg]) {
        float* dst = a.Z + (size_t)nrow[fg] * LAT;
        *reinterpret_cast<f32x4*>(dst + 4 * q) = f32x4{z[fg][0], z[fg][1], z[fg][2], z[fg][3]};
        *reinterpret_cast<f32x4*>(dst + 16 + 4 * q) = f32x4{z[fg][4], z[fg][5], z[fg][6], z[fg][7]};
      }
  }
}

// The chain kernels' noise streams written to global memory (test aid): thread <-> (frame of the tile, latent quad) with
// qpf quads per frame and rows of `width` floats -- 8 and LAT for mh_chain_kernel::draw over the team tiles, 32 and 128
// for widechain_kernel (wide.hip) over the wave tiles; blockDim = qpf * frames of a tile.  (A run-time divide where the two
// kernels had shifts: a test aid, not a hot path.)
__global__ void rng_fill_kernel(const int32_t* tile_utt, const int32_t* tile_n0, const int32_t* tile_cnt,
                                const int32_t* frame_off, const uint64_t* utt_seed, uint32_t call, int S, int NT,
                                int qpf, int width, float* eps_out, float* u_out) {
  const int tile = blockIdx.x, sid = threadIdx.x, sfr = sid / qpf, squad = sid - sfr * qpf;
  const int utt = tile_utt[tile], n0 = tile_n0[tile], cnt = tile_cnt[tile];
  if (sfr >= cnt) return;
  Xs128 st = xs_seed(utt_seed[utt], (uint32_t)(n0 - frame_off[utt] + sfr), (uint32_t)squad, call);
  for (int s = 0; s < S; ++s) {
    const f32x4 e = normal4(st);
    const size_t row = (size_t)s * NT + n0 + sfr;
    *reinterpret_cast<f32x4*>(eps_out + row * width + 4 * squad) = e;
    if (squad == 0) u_out[row] = uniform01(st);
  }
}

// ============================================================================
// Sample decode + fused epilogues (compute_Vs mcem.py:444-454, M_step :90-152,
// cost :68-70, compute_WF :486-488)
// ============================================================================
enum { MODE_STORE = 0, MODE_WSTATS = 1, MODE_HG = 2, MODE_WF = 3,
       MODE_G = 4 };   // gain update + cost only: the M-step of the *_noNMF variants (mcem.py:543-578)

struct DecodeArgs {
  DecW dw;
  const float *X2, *W, *B1, *Zs, *normW, *X;
  const float* Vb;                     // external noise variance [NT][Fs] (noNMF variants) or null
  float *Ht, *g;                       // read (and written by MODE_HG)
  float *Vs_out, *A1, *P, *S_hat, *N_hat, *WFs, *WFn;
  double* cost_frames;
  const int32_t *tile_utt, *tile_n0, *tile_cnt;   // frame tiles (<= 32 NTEAM frames of one utterance each)
  int Fs, K, NT, Rcap, R, n_tiles;
  int w3_lds_off;
  int wl_lds_off;                      // LDS offset of the staged W[utt] (rank <= 8)
};

struct DecodeX {            // one per team
  float redH[8][64];        // [wave][2*Kp]
  float redG[8][2];
  double redC[2][8];        // [iteration parity][wave]
};

template <int NW, int NTEAM, int MT, bool SPLIT, bool W3LDS, int MODE, int KP>
__global__ __launch_bounds__(NW * NTEAM * 64) void decode_kernel(const DecodeArgs a) {
  constexpr int MAXT = MT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using M = LdsMap<NTEAM, SPLIT>;
  constexpr int TPW = NT_H / NW;
  constexpr int Kp = KP;
  const DecW& dw = a.dw;
  const Dec<NW, NTEAM, MT, SPLIT, W3LDS> d = dec_setup<NW, NTEAM, MT, SPLIT, W3LDS>(smem, dw, a.w3_lds_off, a.Fs);
  DecodeX& L = reinterpret_cast<DecodeX*>(smem + M::common_end)[d.team];
  const int lane = threadIdx.x & 63, w = d.w, q = lane >> 4, c = lane & 15;
  const int nch = (a.R + 31) / 32;
  const float* b3l = reinterpret_cast<const float*>(smem + M::b3);
  __syncthreads();

  int fidx[MAXT];
  bool fval[MAXT];
#pragma unroll
  for (int i = 0; i < MAXT; ++i) {
    const int t16 = w + NW * i;
    fidx[i] = 16 * t16 + c;
    fval[i] = d.tile_ok(i) && fidx[i] < dw.Fm;
  }
  // Rank <= 8: the utterance's W (Fs x 8 floats) sits in LDS (every lane reads its bins' rows several times
  // per frame; from L2 each read is an exposed ~2 us round trip for a team that has nothing else to run).
  constexpr bool WLDS = (KP == 8) && MODE != MODE_STORE && MODE != MODE_G;
  float* wl = reinterpret_cast<float*>(smem + a.wl_lds_off);

  // Inputs of one frame.  The ones layer 1 needs at once (latents, M2: the folded layer-1 bias) are loaded
  // one frame ahead, under the previous frame's decode; the rest is issued at the top of the frame and
  // first used after the hidden layers.
  struct FrameIn {
    float zz[2][8];        // first 32 samples' latents, fragment order
    f32x4 b1v[TPW];        // layer-1 accumulator init (M2)
  };
  struct FrameLate {
    float x2f[MT];
    float hrow[KP];
    float g;
    float x2n;             // X2 of the odd last bin
  };
  f32x4 bias1_m1[TPW];                             // M1: the layer-1 bias is the same for every frame
#pragma unroll
  for (int ti = 0; ti < TPW; ++ti) bias1_m1[ti] = *reinterpret_cast<const f32x4*>(dw.b1 + 16 * (w + NW * ti) + 4 * q);

  // ==== frame driver (every mode): tile loop, W staging, input prefetch, per-bin constants, decode_tiles / decode_chunk ====
  // one tile (frames of one utterance) at a time; the teams take alternate frames of the tile
  for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
  const int utt = a.tile_utt[tile];
  const int n_beg = a.tile_n0[tile], n_end = n_beg + a.tile_cnt[tile];
  if (WLDS) {
    if (tile != (int)blockIdx.x) __syncthreads();          // every wave is done with the previous tile's W
    const f32x4* src = reinterpret_cast<const f32x4*>(a.W + (size_t)utt * a.Fs * KP);
    for (int e = threadIdx.x; e < a.Fs * KP / 4; e += blockDim.x) reinterpret_cast<f32x4*>(wl)[e] = src[e];
    __syncthreads();
  }
  auto frame_of = [&](int nb, bool& on) {
    on = nb + d.team < n_end;                   // team without a frame shadows the last one, stores masked
    return on ? nb + d.team : n_end - 1;
  };
  auto load_z = [&](int n, int ch, float (&zz)[2][8]) {
#pragma unroll
    for (int sg = 0; sg < 2; ++sg) {
      int r = 32 * ch + 16 * sg + c;
      r = r < a.R ? r : a.R - 1;
      const float* src = a.Zs + ((size_t)n * a.Rcap + r) * LAT;
      const f32x4 lo = *reinterpret_cast<const f32x4*>(src + 4 * q);
      const f32x4 hi = *reinterpret_cast<const f32x4*>(src + 16 + 4 * q);
#pragma unroll
      for (int t = 0; t < 4; ++t) { zz[sg][t] = lo[t]; zz[sg][4 + t] = hi[t]; }
    }
  };
  auto load_frame = [&](int n, FrameIn& f) {
    load_z(n, 0, f.zz);
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti)
      f.b1v[ti] = a.B1 ? *reinterpret_cast<const f32x4*>(a.B1 + (size_t)n * HID + 16 * (w + NW * ti) + 4 * q) : bias1_m1[ti];
  };
  auto load_late = [&](int n, FrameLate& f) {
    if (MODE != MODE_STORE) {
      f.g = a.g[n];
      f.x2n = d.nyq ? a.X2[(size_t)n * a.Fs + dw.F - 1] : 0.f;
#pragma unroll
      for (int i = 0; i < MT; ++i) f.x2f[i] = (d.tile_ok(i)) ? a.X2[(size_t)n * a.Fs + fidx[i]] : 0.f;
#pragma unroll
      for (int k = 0; k < KP; k += 4) {
        const f32x4 hv = *reinterpret_cast<const f32x4*>(a.Ht + (size_t)n * KP + k);
#pragma unroll
        for (int t = 0; t < 4; ++t) f.hrow[k + t] = hv[t];
      }
    }
  };
  // (MODE_HG keeps every sample variance of the frame in registers: the second input set only fits at rank 8, bf16)
  constexpr bool HEAVY = MODE == MODE_HG || MODE == MODE_G;
  constexpr bool PREFETCH = HEAVY ? (!SPLIT && KP == 8) : true;
  FrameIn nxt;
  if (PREFETCH) {
    bool on0;
    load_frame(frame_of(n_beg, on0), nxt);
  }
  int pend_n = -1, pend_par = 0, cpar = 0;        // MODE_HG: frame whose cost partials wait in LDS
  auto finish_cost = [&]() {
    if ((MODE == MODE_HG || MODE == MODE_G) && pend_n >= 0 && w == 0 && lane == 0) {
      double s = 0.0;
      for (int ww = 0; ww < NW; ++ww) s += L.redC[pend_par][ww];
      a.cost_frames[pend_n] = s;
    }
    pend_n = -1;
  };
  for (int nb = n_beg; nb < n_end; nb += NTEAM) {
    bool on;
    const int n = frame_of(nb, on);
    if (!PREFETCH) load_frame(n, nxt);
    const FrameIn cur = nxt;
    FrameLate late;
    load_late(n, late);
    if (PREFETCH && nb + NTEAM < n_end) {
      bool on2;
      load_frame(frame_of(nb + NTEAM, on2), nxt);
    }
    VN_STAMP_DECL
    f32x4 bias1[TPW][2];
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti) {
      bias1[ti][0] = cur.b1v[ti];
      bias1[ti][1] = bias1[ti][0];
    }
    // decode 32 samples (chunk ch) of frame n: vs[i][sg][t] = Vs(sample 32ch+16sg+4q+t, bin fidx[i])
    float vsn[2] = {0.f, 0.f}, mkn[2] = {0.f, 0.f};   // odd last bin, column-on-lane: Vs and validity of sample (sg, c)
    float mk[2][4];                    // 1 for real samples of chunk 0, 0 for the padding columns
#pragma unroll
    for (int sg = 0; sg < 2; ++sg)
#pragma unroll
      for (int t = 0; t < 4; ++t) mk[sg][t] = (16 * sg + 4 * q + t < a.R) ? 1.f : 0.f;
    auto rvalid = [&](int ch, int sg, int t) { return 32 * ch + 16 * sg + 4 * q + t < a.R; };
    // ---- per-bin constants of frame n: X2, rows of W, Vb = sum_k W[f,k] H[k,n]
    // (computing them after the hidden layers, when their loads have surely landed, measured slower:
    // wstats 0.316 -> 0.330 ms, H/g 0.602 -> 0.614 ms)
    const float gn_late = late.g;
    float x2f[MAXT], vb[MAXT];
    auto wrow = [&](int i, int k) {   // 4 consecutive ranks of W[utt][fidx[i]][:]
      if (WLDS) return *reinterpret_cast<const f32x4*>(wl + fidx[i] * KP + k);
      return *reinterpret_cast<const f32x4*>(a.W + ((size_t)utt * a.Fs + fidx[i]) * Kp + k);
    };
    auto dotWH = [&](int i, const float (&hvec)[KP]) {
      float v = 0.f;
#pragma unroll
      for (int k = 0; k < Kp; k += 4) {
        const f32x4 ww = wrow(i, k);
        v += ww[0] * hvec[k] + ww[1] * hvec[k + 1] + ww[2] * hvec[k + 2] + ww[3] * hvec[k + 3];
      }
      return v;
    };
    // W[utt][F-1][:] (odd last bin), re-read at its three uses (same address in every lane: one L1 line)
    auto wn4 = [&](int k) {
      if (WLDS) return *reinterpret_cast<const f32x4*>(wl + (dw.F - 1) * KP + k);
      return *reinterpret_cast<const f32x4*>(a.W + ((size_t)utt * a.Fs + dw.F - 1) * Kp + k);
    };
    float hs[KP];   // H[:,n] (MODE_HG: times the pending column norms of W)
    float vbn = 1.f, gn = 1.f, x2n = 0.f;
    if (MODE != MODE_STORE) {
      gn = gn_late;
      x2n = late.x2n;
#pragma unroll
      for (int k = 0; k < Kp; k += 4) {
        f32x4 nv = {1.f, 1.f, 1.f, 1.f};
        if (MODE == MODE_HG) nv = *reinterpret_cast<const f32x4*>(a.normW + (size_t)utt * Kp + k);   // (MODE_G: H is not used)
#pragma unroll
        for (int t = 0; t < 4; ++t) hs[k + t] = late.hrow[k + t] * nv[t];
      }
#pragma unroll
      for (int i = 0; i < MAXT; ++i) {
        const bool tv = d.tile_ok(i);
        x2f[i] = late.x2f[i];
        vb[i] = !tv ? 1.f : (a.Vb ? a.Vb[(size_t)n * a.Fs + fidx[i]] : dotWH(i, hs));
      }
      if (d.nyq && a.Vb) {
        vbn = a.Vb[(size_t)n * a.Fs + dw.F - 1];
      } else if (d.nyq) {
        vbn = 0.f;
#pragma unroll
        for (int k = 0; k < Kp; k += 4) {
          const f32x4 ww = wn4(k);
          vbn += ww[0] * hs[k] + ww[1] * hs[k + 1] + ww[2] * hs[k + 2] + ww[3] * hs[k + 3];
        }
      }
    }
    // decode 32 samples (chunk ch) of frame n; each finished bin tile i is handed to epi(i, vs0, vs1) with
    // vs_sg[t] = Vs(sample 32ch+16sg+4q+t, bin fidx[i]) so its VALU work overlaps the next tile's MFMAs
    auto decode_tiles = [&](int ch, auto epi) {
      bf16x8 zhi[2], zlo[2];
      if (ch == 0) {
        split8<SPLIT>(cur.zz[0], zhi[0], zlo[0]);
        split8<SPLIT>(cur.zz[1], zhi[1], zlo[1]);
      } else {
        float zz[2][8];
        load_z(n, ch, zz);
        split8<SPLIT>(zz[0], zhi[0], zlo[0]);
        split8<SPLIT>(zz[1], zhi[1], zlo[1]);
      }
      // bf16x3 mode: the two layer images alias, so layer 1 below overwrites what the previous call's output layer reads.
      // Nothing else orders the two: a wavefront that owns fewer bin tiles than its neighbours (NT3 not a multiple of
      // the team's wavefronts; every F = 16k+1 of a power-of-two STFT divides evenly) got here while they were reading.
      if (M::ALIAS) d.team_sync();
      d.hidden(zhi, zlo, bias1, []() {});
      if (d.nyq) {
        const float bn = b3l[dw.F - 1];
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) {
          vsn[sg] = fast_exp(d.nyq_logit(sg, bn));
          mkn[sg] = (32 * ch + 16 * sg + c < a.R) ? 1.f : 0.f;
        }
      }
      // (the k-step-major form measured faster here than Dec::out_bins_by_frames' tile-major one: wstats 0.303 vs 0.312 ms)
      f32x4 va[MAXT][2];
#pragma unroll
      for (int i = 0; i < MAXT; ++i) {
        const float bv = d.tile_ok(i) ? b3l[fidx[i]] : 0.f;
        va[i][0] = f32x4{bv, bv, bv, bv};
        va[i][1] = va[i][0];
      }
      d.out_samples_by_bins(va);
#pragma unroll
      for (int i = 0; i < MAXT; ++i)
        if (d.tile_ok(i)) {
#pragma unroll
          for (int t = 0; t < 4; ++t) { va[i][0][t] = fast_exp(va[i][0][t]); va[i][1][t] = fast_exp(va[i][1][t]); }
          epi(i, va[i][0], va[i][1]);
        }
    };
    auto decode_chunk = [&](int ch, f32x4 (&vs)[MAXT][2]) {
#pragma unroll
      for (int i = 0; i < MAXT; ++i) { vs[i][0] = f32x4{1.f, 1.f, 1.f, 1.f}; vs[i][1] = vs[i][0]; }   // tiles this wave does not own
      decode_tiles(ch, [&](int i, const f32x4 v0, const f32x4 v1) { vs[i][0] = v0; vs[i][1] = v1; });
    };
    const bool lead = w == 0 && lane == 0;            // the one lane that books the odd last bin
    auto sum_q = [&](float v) { return sum_rows4(v); };
    auto sum_c = [&](float v) { return sum_row16(v); };

    // ==== the modes.  Tile values are vs[i][sg][t] with vb[i] and the sample mask, summed over q; the odd last bin is
    // column-on-lane -- vsn[sg] with vbn and mkn[sg], summed over c -- and follows each tile pass as its scalar twin.
    // (The twins stay written out: shared through lambdas they changed registers and speed) ====
    // ---- MODE_STORE (compute_Vs, mcem.py:444-454): the variances themselves, zeros in the padding bins
    if (MODE == MODE_STORE) {
      for (int ch = 0; ch < nch; ++ch) {
        f32x4 vs[MAXT][2];
        decode_chunk(ch, vs);
        if (on) {
#pragma unroll
          for (int i = 0; i < MAXT; ++i)
            if (d.tile_ok(i))
#pragma unroll
              for (int sg = 0; sg < 2; ++sg)
#pragma unroll
                for (int t = 0; t < 4; ++t)
                  if (rvalid(ch, sg, t))
                    a.Vs_out[((size_t)n * a.R + 32 * ch + 16 * sg + 4 * q + t) * a.Fs + fidx[i]] = fval[i] ? vs[i][sg][t] : 0.f;
          if (d.nyq && w == 0 && q == 0)
#pragma unroll
            for (int sg = 0; sg < 2; ++sg)
              if (mkn[sg] != 0.f) {
                float* row = a.Vs_out + ((size_t)n * a.R + 32 * ch + 16 * sg + c) * a.Fs;
                row[dw.F - 1] = vsn[sg];
                for (int f = dw.F; f < a.Fs; ++f) row[f] = 0.f;       // padding bins
              }
        }
      }
      continue;
    }

    // ---- MODE_WSTATS
    if (MODE == MODE_WSTATS) {
      // A1 = sum_r 1/Vx, A2 = sum_r 1/Vx^2 with the pre-update variances (mcem.py:107-109)
      float a1[MAXT], a2[MAXT], a1n = 0.f, a2n = 0.f;
#pragma unroll
      for (int i = 0; i < MAXT; ++i) a1[i] = a2[i] = 0.f;
      for (int ch = 0; ch < nch; ++ch) {
        decode_tiles(ch, [&](int i, const f32x4 v0, const f32x4 v1) {
#pragma unroll
          for (int sg = 0; sg < 2; ++sg)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              const float v = sg == 0 ? v0[t] : v1[t];
              const float r = fast_rcp(gn * v + vb[i]) * (ch == 0 ? mk[sg][t] : (rvalid(ch, sg, t) ? 1.f : 0.f));
              a1[i] += r;
              a2[i] += r * r;
            }
        });
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) {
          const float r = fast_rcp(gn * vsn[sg] + vbn) * mkn[sg];
          a1n += r;
          a2n += r * r;
        }
      }
#pragma unroll
      for (int i = 0; i < MAXT; ++i) {
        const float s1 = sum_q(a1[i]), s2 = sum_q(a2[i]);
        if (on && q == 0 && d.tile_ok(i)) {
          a.A1[(size_t)n * a.Fs + fidx[i]] = fval[i] ? s1 : 0.f;
          a.P[(size_t)n * a.Fs + fidx[i]] = fval[i] ? x2f[i] * s2 : 0.f;
        }
      }
      if (d.nyq) {
        const float s1 = sum_c(a1n), s2 = sum_c(a2n);
        if (on && w == 0 && q == 0 && dw.F - 1 + c < a.Fs) {       // lane 0: the bin; lanes 1..: zero the padding
          a.A1[(size_t)n * a.Fs + dw.F - 1 + c] = c == 0 ? s1 : 0.f;
          a.P[(size_t)n * a.Fs + dw.F - 1 + c] = c == 0 ? x2n * s2 : 0.f;
        }
      }
    // ---- MODE_WF
    } else if (MODE == MODE_WF) {
      // WFs = mean_r(g Vs / Vx), WFn = mean_r(Vb / Vx)  (mcem.py:486-488)
      float ws[MAXT], wn[MAXT], wsn = 0.f, wnn = 0.f;
#pragma unroll
      for (int i = 0; i < MAXT; ++i) ws[i] = wn[i] = 0.f;
      for (int ch = 0; ch < nch; ++ch) {
        f32x4 vs[MAXT][2];
        decode_chunk(ch, vs);
#pragma unroll
        for (int i = 0; i < MAXT; ++i)
#pragma unroll
          for (int sg = 0; sg < 2; ++sg)
#pragma unroll
            for (int t = 0; t < 4; ++t)
              if (rvalid(ch, sg, t)) {
                const float sc = gn * vs[i][sg][t];
                const float r = fast_rcp(sc + vb[i]);
                ws[i] += sc * r;
                wn[i] += vb[i] * r;
              }
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) {
          const float sc = gn * vsn[sg];
          const float r = fast_rcp(sc + vbn) * mkn[sg];
          wsn += sc * r;
          wnn += vbn * r;
        }
      }
      const float invR = 1.0f / (float)a.R;
      if (d.nyq) {
        const float s = sum_c(wsn) * invR, nn = sum_c(wnn) * invR;
        if (on && w == 0 && q == 0 && dw.F - 1 + c < a.Fs) {       // lane 0: the bin; lanes 1..: zero the padding
          const size_t o = (size_t)n * a.Fs + dw.F - 1 + c;
          const float ms = c == 0 ? s : 0.f, mn = c == 0 ? nn : 0.f;
          const float xr = a.X[2 * o], xi = a.X[2 * o + 1];
          a.S_hat[2 * o] = ms * xr;  a.S_hat[2 * o + 1] = ms * xi;
          a.N_hat[2 * o] = mn * xr;  a.N_hat[2 * o + 1] = mn * xi;
          if (a.WFs) a.WFs[o] = ms;
          if (a.WFn) a.WFn[o] = mn;
        }
      }
#pragma unroll
      for (int i = 0; i < MAXT; ++i) {
        const float s = sum_q(ws[i]) * invR, nn = sum_q(wn[i]) * invR;
        if (on && q == 0 && d.tile_ok(i)) {
          const size_t o = (size_t)n * a.Fs + fidx[i];
          const float xr = a.X[2 * o], xi = a.X[2 * o + 1];
          a.S_hat[2 * o] = fval[i] ? s * xr : 0.f;  a.S_hat[2 * o + 1] = fval[i] ? s * xi : 0.f;   // mcem.py:175
          a.N_hat[2 * o] = fval[i] ? nn * xr : 0.f; a.N_hat[2 * o + 1] = fval[i] ? nn * xi : 0.f;  // mcem.py:176
          if (a.WFs) a.WFs[o] = fval[i] ? s : 0.f;
          if (a.WFn) a.WFn[o] = fval[i] ? nn : 0.f;
        }
      }
    // ---- MODE_HG: H, variances with the new H, g, cost; MODE_G (fixed noise model): g and cost only
    } else if (MODE == MODE_HG || MODE == MODE_G) {
      f32x4 vs[MAXT][2];
      // chunk validity mask (chunk 0 uses mk; later chunks are rare: R > 32)
      auto mask = [&](int ch, int sg, int t) { return ch == 0 ? mk[sg][t] : (rvalid(ch, sg, t) ? 1.f : 0.f); };
      float vbn2 = vbn;
      if (MODE == MODE_G) {
        if (nch == 1) decode_chunk(0, vs);
      } else {
      // ---- H update (mcem.py:118-121): W already updated + normalised by w_update_kernel
      float a1[MAXT], a2[MAXT], a1n = 0.f, a2n = 0.f;
#pragma unroll
      for (int i = 0; i < MAXT; ++i) a1[i] = a2[i] = 0.f;
      VN_STAMP_AT(0);
      for (int ch = 0; ch < nch; ++ch) {
        decode_tiles(ch, [&](int i, const f32x4 v0, const f32x4 v1) {
          vs[i][0] = v0;
          vs[i][1] = v1;
#pragma unroll
          for (int sg = 0; sg < 2; ++sg)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              const float r = fast_rcp(gn * (sg == 0 ? v0[t] : v1[t]) + vb[i]) * mask(ch, sg, t);
              a1[i] += r;
              a2[i] += r * r;
            }
        });
        VN_STAMP_AT(1);
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) {
          const float r = fast_rcp(gn * vsn[sg] + vbn) * mkn[sg];
          a1n += r;
          a2n += r * r;
        }
      }
#pragma unroll
      for (int i = 0; i < MAXT; ++i) {
        const float s1 = sum_q(a1[i]), s2 = sum_q(a2[i]);
        a1[i] = fval[i] ? s1 : 0.f;
        a2[i] = fval[i] ? s2 * x2f[i] : 0.f;
      }
      if (d.nyq) { a1n = sum_c(a1n); a2n = sum_c(a2n) * x2n; }
      VN_STAMP_AT(2);
      // num_k = sum_f W[f,k] X2 A2, den_k = sum_f W[f,k] A1: in-lane over this wave's bins, DPP row sum
      // over the 16 bins of a tile, one LDS hop over the waves
      // (ranks in groups of 8 so that a large rank does not need 2*KP live accumulators)
#pragma unroll
      for (int k0 = 0; k0 < Kp; k0 += 8) {
        float nuk[8], dek[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) nuk[k] = dek[k] = 0.f;
#pragma unroll
        for (int i = 0; i < MAXT; ++i)
          if (d.tile_ok(i)) {
#pragma unroll
            for (int k = 0; k < 8; k += 4) {
              const f32x4 ww = wrow(i, k0 + k);
#pragma unroll
              for (int t = 0; t < 4; ++t) { nuk[k + t] += ww[t] * a2[i]; dek[k + t] += ww[t] * a1[i]; }
            }
          }
        if (d.nyq && lead) {
#pragma unroll
          for (int k = 0; k < 8; k += 4) {
            const f32x4 ww = wn4(k0 + k);
#pragma unroll
            for (int t = 0; t < 4; ++t) { nuk[k + t] += ww[t] * a2n; dek[k + t] += ww[t] * a1n; }
          }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) { nuk[k] = sum_c(nuk[k]); dek[k] = sum_c(dek[k]); }
        if (lane == 0) {
#pragma unroll
          for (int k = 0; k < 8; k += 4) {
            *reinterpret_cast<f32x4*>(&L.redH[w][k0 + k]) = f32x4{nuk[k], nuk[k + 1], nuk[k + 2], nuk[k + 3]};
            *reinterpret_cast<f32x4*>(&L.redH[w][32 + k0 + k]) = f32x4{dek[k], dek[k + 1], dek[k + 2], dek[k + 3]};
          }
        }
      }
      VN_STAMP_AT(3);
      d.team_sync();
      VN_STAMP_AT(4);
      finish_cost();
      float hn[KP];
#pragma unroll
      for (int k = 0; k < Kp; k += 4) {
        f32x4 nu = {0, 0, 0, 0}, de = {0, 0, 0, 0};
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) {
          nu += *reinterpret_cast<const f32x4*>(&L.redH[ww][k]);
          de += *reinterpret_cast<const f32x4*>(&L.redH[ww][32 + k]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
          hn[k + t] = (k + t < a.K) ? hs[k + t] * __builtin_amdgcn_sqrtf(nu[t] * fast_rcp(de[t])) : 0.f;   // mcem.py:121
      }
      if (on && w == 0 && lane == 0) {
#pragma unroll
        for (int k = 0; k < Kp; k += 4)
          *reinterpret_cast<f32x4*>(a.Ht + (size_t)n * Kp + k) = f32x4{hn[k], hn[k + 1], hn[k + 2], hn[k + 3]};
      }
      VN_STAMP_AT(5);
      // ---- variances with the new W, H (mcem.py:124-125)
#pragma unroll
      for (int i = 0; i < MAXT; ++i) vb[i] = (d.tile_ok(i)) ? dotWH(i, hn) : 1.f;
      if (d.nyq) {
        vbn2 = 0.f;
#pragma unroll
        for (int k = 0; k < Kp; k += 4) {
          const f32x4 ww = wn4(k);
          vbn2 += ww[0] * hn[k] + ww[1] * hn[k + 1] + ww[2] * hn[k + 2] + ww[3] * hn[k + 3];
        }
      }
      }   // MODE_HG
      // ---- g update (mcem.py:138-142 / :564-568)
      float ng[MAXT], dg[MAXT], ngn = 0.f, dgn = 0.f;
#pragma unroll
      for (int i = 0; i < MAXT; ++i) ng[i] = dg[i] = 0.f;
      for (int ch = 0; ch < nch; ++ch) {
        if (nch > 1) decode_chunk(ch, vs);
#pragma unroll
        for (int i = 0; i < MAXT; ++i)
#pragma unroll
          for (int sg = 0; sg < 2; ++sg)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              const float v = vs[i][sg][t];
              const float r = fast_rcp(gn * v + vb[i]) * mask(ch, sg, t);
              const float vr = v * r;
              dg[i] += vr;            // sum_r Vs / Vx
              ng[i] += vr * r;        // sum_r Vs / Vx^2
            }
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) {
          const float r = fast_rcp(gn * vsn[sg] + vbn2) * mkn[sg];
          const float vr = vsn[sg] * r;
          dgn += vr;
          ngn += vr * r;
        }
      }
      float nu = 0.f, de = 0.f;
#pragma unroll
      for (int i = 0; i < MAXT; ++i) {
        const float sn = sum_q(ng[i]), sdn = sum_q(dg[i]);
        if (fval[i]) { nu += x2f[i] * sn; de += sdn; }
      }
      if (d.nyq) {
        const float sn = sum_c(ngn), sdn = sum_c(dgn);
        if (lead) { nu += x2n * sn; de += sdn; }
      }
      nu = sum_c(nu);
      de = sum_c(de);
      VN_STAMP_AT(6);
      if (lane == 0) { L.redG[w][0] = nu; L.redG[w][1] = de; }
      d.team_sync();
      VN_STAMP_AT(7);
      if (MODE == MODE_G) finish_cost();
      nu = de = 0.f;
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) { nu += L.redG[ww][0]; de += L.redG[ww][1]; }
      const float gnew = gn * __builtin_amdgcn_sqrtf(nu * fast_rcp(de));          // mcem.py:142
      if (on && w == 0 && lane == 0) a.g[n] = gnew;
      // ---- cost (mcem.py:70) with the refreshed variances (mcem.py:151-152)
      float cs = 0.f, csn = 0.f;
      for (int ch = 0; ch < nch; ++ch) {
        if (nch > 1) decode_chunk(ch, vs);
#pragma unroll
        for (int i = 0; i < MAXT; ++i) {
          float cl = 0.f, cx = 0.f;                         // sum log2 Vx, sum 1/Vx over this lane's samples
#pragma unroll
          for (int sg = 0; sg < 2; ++sg)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              const float vx = gnew * vs[i][sg][t] + vb[i];
              const float m = mask(ch, sg, t);
              cl += fast_log2(vx) * m;
              cx += fast_rcp(vx) * m;
            }
          cs += fval[i] ? cl * LN2_F + x2f[i] * cx : 0.f;
        }
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) {
          const float vx = gnew * vsn[sg] + vbn2;
          csn += (fast_log(vx) + x2n * fast_rcp(vx)) * mkn[sg];
        }
      }
      if (d.nyq) {
        const float t = sum_c(csn);
        if (lead) cs += t;
      }
      // wave sum: rows in fp32 (DPP), then fp64 across the 4 rows and the waves
      double cd = sum_rows4_d((double)sum_c(cs));
      VN_STAMP_AT(8);
      // the cross-wave sum of the cost is finished one iteration later (after that iteration's first
      // barrier) so that this reduction costs no barrier of its own
      if (lane == 0) L.redC[cpar][w] = cd;
      pend_n = on ? n : -1;
      pend_par = cpar;
      cpar ^= 1;
      VN_STAMP_AT(9);
    }
  }
  if (MODE == MODE_HG || MODE == MODE_G) {
    d.team_sync();
    finish_cost();
  }
  }   // tiles
}

}  // namespace

// ============================================================================
// Host launchers (C ABI)
// ============================================================================
namespace {

DecW make_decw(const vaenmf_plan* p) {
  DecW d;
  d.w1f = p->w1f; d.w2f = p->w2f; d.w3f = p->w3f;
  d.b1 = p->b1; d.b2 = p->b2; d.b3 = p->b3;
  d.NT3 = p->NT3; d.F = p->cfg.F; d.Fm = p->Fm; d.w3n = p->w3n;
  d.Lz = p->Lz; d.one_hidden = p->one_hidden ? 1 : 0;
  return d;
}

// LDS bytes and W3 placement: W3 fragments go to LDS when they fit, else stream from L2
template <int NTEAM, bool SPLIT>
void lds_plan(int NT3, size_t extra_per_team, int* w3_off, size_t* total) {
  using M = LdsMap<NTEAM, SPLIT>;
  const size_t base = (M::common_end + NTEAM * extra_per_team + 15) / 16 * 16;
  const size_t w3 = M::w3_bytes(NT3);
  if (base + w3 <= (size_t)VN_LDS_LIMIT) { *w3_off = (int)base; *total = base + w3; }
  else { *w3_off = -1; *total = base; }
}

template <int V> using ic = std::integral_constant<int, V>;
// The one switch over the workgroup geometry and the precision: fn(ic<NW>, ic<NTEAM>, ic<MT>, bool_constant<SPLIT>).
// plan.hip picks the geometry from the number of bin tiles NT3 of the MFMA path:
//   0 = 2 teams x 4 waves, 5 bin tiles per wave (NT3 <= 20)      3 = 2 teams x 4 waves, 4 tiles (NT3 == 16)
//   2 = 1 team  x 8 waves, 5 bin tiles per wave (NT3 <= 40)      4 = 1 team  x 8 waves, 4 tiles (NT3 == 32)
template <typename FN>
int with_geom(const vaenmf_plan* p, FN fn) {
  auto prec = [&](auto nw, auto nteam, auto mt) {
    return p->cfg.precision == VAENMF_PREC_BF16X3 ? fn(nw, nteam, mt, std::true_type{}) : fn(nw, nteam, mt, std::false_type{});
  };
  switch (p->geom) {
    case 0: return prec(ic<4>{}, ic<2>{}, ic<5>{});
    case 3: return prec(ic<4>{}, ic<2>{}, ic<4>{});
    case 4: return prec(ic<8>{}, ic<1>{}, ic<4>{});
    default: return prec(ic<8>{}, ic<1>{}, ic<5>{});
  }
}
// ensure the dynamic LDS, then launch the W3LDS instantiation that a.w3_lds_off selects; kern(bool_constant<W3LDS>) names it
template <typename KERN, typename ARGS>
int launch_w3(KERN kern, const ARGS& a, int grid, int threads, size_t lds, hipStream_t st) {
  auto go = [&](auto* fn) -> int {
    if (int e = vn_ensure_dyn_lds((const void*)fn, VN_LDS_LIMIT)) return e;
    hipLaunchKernelGGL(fn, dim3(grid), dim3(threads), lds, st, a);
    return 0;
  };
  return a.w3_lds_off >= 0 ? go(kern(std::true_type{})) : go(kern(std::false_type{}));
}

template <int MODE>
int launch_decode(const vaenmf_plan* p, DecodeArgs a, hipStream_t st) {
  const int want = p->n_sms * 2;
  int grid = a.n_tiles < want ? a.n_tiles : want;
  const int cap = vn_switches().grid_cap;               // (tests: a small grid makes every workgroup walk several tiles)
  if (cap > 0 && cap < grid) grid = cap;
  const int Kp = (MODE == MODE_STORE) ? 8 : p->Kp;
  return with_geom(p, [&](auto nw, auto nteam, auto mt, auto split) -> int {
    constexpr int NW = decltype(nw)::value, NTEAM = decltype(nteam)::value, MT = decltype(mt)::value;
    constexpr bool SPLIT = decltype(split)::value;
    size_t lds;
    // per team: DecodeX; per workgroup: the staged W[utt] (rank <= 8), placed right after the DecodeX blocks
    const size_t wl_bytes = (Kp == 8 && MODE != MODE_STORE && MODE != MODE_G) ? (size_t)a.Fs * 8 * sizeof(float) : 0;
    const size_t x_bytes = (NTEAM * sizeof(DecodeX) + 15) / 16 * 16;
    lds_plan<NTEAM, SPLIT>(a.dw.NT3, (x_bytes + wl_bytes + NTEAM - 1) / NTEAM, &a.w3_lds_off, &lds);
    a.wl_lds_off = (int)(LdsMap<NTEAM, SPLIT>::common_end + x_bytes);
    auto rank = [&](auto kp) {
      return launch_w3([](auto w3) { return &decode_kernel<NW, NTEAM, MT, SPLIT, decltype(w3)::value, MODE, decltype(kp)::value>; },
                       a, grid, NW * NTEAM * 64, lds, st);
    };
    return Kp == 8 ? rank(ic<8>{}) : (Kp == 16 ? rank(ic<16>{}) : rank(ic<32>{}));
  });
}

DecodeArgs base_decode_args(const vaenmf_plan* p, const float* Zs, int Rcap, int R, const float* B1) {
  DecodeArgs a = {};
  a.dw = make_decw(p);
  a.Zs = Zs; a.B1 = B1; a.tile_utt = p->d_tile_utt; a.tile_n0 = p->d_tile_n0; a.tile_cnt = p->d_tile_cnt; a.n_tiles = p->n_tiles;
  a.Fs = p->Fs; a.K = p->cfg.K; a.NT = p->NT; a.Rcap = Rcap; a.R = R; a.Vb = p->Vb_ext;
  return a;
}

// the step-wise decoding entry points have no wide form
int require_narrow(const vaenmf_plan* p, const char* entry) {
  VN_REQUIRE(!p->wide, "%s: a wide decoder plan (z_dim > 32 or a hidden layer of 256 units) has no decoding kernels; run the chain with the sample "
             "store on (vaenmf_sample_store) and use vaenmf_m_step_stored / vaenmf_wiener_stored (vaenmf_sample_store_gather for the variances)", entry);
  return 0;
}

}  // namespace

// the team chain of one MH-chain call, the mirror of chain.hip's vn_launch_wchain: kernel arguments from the plan and the
// call, then the workgroup geometry
int vn_launch_tchain(vaenmf_plan* p, const VnChainCall& cc, hipStream_t st) {
  ChainArgs a = {};
  a.dw = make_decw(p);
  a.X2 = cc.X2; a.W = cc.W; a.Ht = cc.Ht; a.g = cc.g; a.B1 = cc.B1; a.Z = cc.Z; a.Zs = cc.Zs; a.acc_out = cc.acc_out; a.Vb = p->Vb_ext;
  a.VsS = cc.VsS; a.src = cc.src; a.Rs = cc.Rs; a.lay = cc.lay;
  a.tile_utt = p->d_tile_utt; a.tile_n0 = p->d_tile_n0; a.tile_cnt = p->d_tile_cnt; a.frame_off = p->d_frame_off;
  a.utt_seed = p->d_utt_seed; a.eps = cc.eps; a.u = cc.u;
  a.Fs = p->Fs; a.Kp = p->Kp; a.NT = p->NT; a.Rcap = cc.Rcap; a.nsamples = cc.nsamples; a.burnin = cc.burnin;
  a.rng_mode = cc.rng_mode; a.call = cc.call; a.sd = cc.sd; a.update_Z = cc.update_Z;
  const int lrc = with_geom(p, [&](auto nw, auto nteam, auto mt, auto split) -> int {
    constexpr int NW = decltype(nw)::value, NTEAM = decltype(nteam)::value, MT = decltype(mt)::value;
    constexpr bool SPLIT = decltype(split)::value;
    size_t lds;
    lds_plan<NTEAM, SPLIT>(a.dw.NT3, sizeof(ChainX), &a.w3_lds_off, &lds);
    auto store = [&](auto store_on) {
      return launch_w3([](auto w3) { return &mh_chain_kernel<NW, NTEAM, MT, SPLIT, decltype(w3)::value, decltype(store_on)::value>; },
                       a, p->n_tiles, NW * NTEAM * 64, lds, st);
    };
    return cc.VsS ? store(std::true_type{}) : store(std::false_type{});
  });
  if (lrc) return lrc;
  VN_CHECK_HIP(hipGetLastError());
  p->last_chain_kernel = 0;
  return 0;
}

// the one rng_fill_kernel over a plan's tile tables: `frames` frames per tile, Lp / 4 quads of a frame's Lp latents
static int launch_rng_fill(vaenmf_plan* p, int n_tiles, int frames, const int32_t* t_utt, const int32_t* t_n0, const int32_t* t_cnt, uint32_t call,
                           int S, float* eps_out, float* u_out, hipStream_t st) {
  const int qpf = p->Lp / 4;
  hipLaunchKernelGGL(rng_fill_kernel, dim3(n_tiles), dim3(qpf * frames), 0, st, t_utt, t_n0, t_cnt, p->d_frame_off, p->d_utt_seed, call, S, p->NT,
                     qpf, p->Lp, eps_out, u_out);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}
// a wide plan draws per 16-frame wave tile, 32 quads of 128 latents: [S][NT][128]
int vn_launch_wide_rng_fill(vaenmf_plan* p, uint32_t call, int S, float* eps_out, float* u_out, hipStream_t st) {
  return launch_rng_fill(p, p->n_wtiles, 16, p->d_wt_utt, p->d_wt_n0, p->d_wt_cnt, call, S, eps_out, u_out, st);
}

extern "C" int vaenmf_rng_fill(vaenmf_plan* p, uint32_t call, int32_t S, float* eps_out, float* u_out, void* stream) {
  if (int e = check_bound(p)) return e;
  if (p->wide) return vn_launch_wide_rng_fill(p, call, S, eps_out, u_out, (hipStream_t)stream);
  return launch_rng_fill(p, p->n_tiles, p->tile_frames, p->d_tile_utt, p->d_tile_n0, p->d_tile_cnt, call, S, eps_out, u_out, (hipStream_t)stream);   // team tiles, 8 quads of 32
}

extern "C" int vaenmf_decode(vaenmf_plan* p, const float* Zs, int32_t Rcap, int32_t R, const float* B1, float* Vs_out, void* stream) {
  if (int e = check_bound(p)) return e;
  if (int e = require_narrow(p, "vaenmf_decode")) return e;
  VN_REQUIRE(R >= 1 && R <= Rcap, "bad R=%d (Rcap=%d)", R, Rcap);
  DecodeArgs a = base_decode_args(p, Zs, Rcap, R, B1);
  a.Vs_out = Vs_out;
  launch_decode<MODE_STORE>(p, a, (hipStream_t)stream);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int vaenmf_m_step(vaenmf_plan* p, const float* X2, float* W, float* Ht, float* g, const float* Zs,
                             int32_t Rcap, int32_t R, const float* B1, double* cost_frames, void* stream) {
  if (int e = check_bound(p)) return e;
  if (int e = require_narrow(p, "vaenmf_m_step")) return e;
  VN_REQUIRE(R >= 1 && R <= Rcap, "bad R=%d (Rcap=%d)", R, Rcap);
  hipStream_t st = (hipStream_t)stream;
  DecodeArgs a = base_decode_args(p, Zs, Rcap, R, B1);
  a.X2 = X2; a.W = W; a.Ht = Ht; a.g = g; a.A1 = p->A1; a.P = p->P; a.normW = p->normW;
  a.cost_frames = cost_frames ? cost_frames : p->cost_frames;
  if (p->Vb_ext) {                                      // noNMF: only the gains move (mcem.py:543-578)
    ProfScope ps(p, VN_K_HG, st);
    launch_decode<MODE_G>(p, a, st);
    VN_CHECK_HIP(hipGetLastError());
    return 0;
  }
  { ProfScope ps(p, VN_K_WSTATS, st); launch_decode<MODE_WSTATS>(p, a, st); }   // A1, X2*A2 per (frame, bin)
  { ProfScope ps(p, VN_K_WUPDATE, st); if (int e = vn_launch_w_update(p, W, Ht, st)) return e; }  // W <- W sqrt(num/den), L1 norms
  { ProfScope ps(p, VN_K_HG, st); launch_decode<MODE_HG>(p, a, st); }           // H, g, cost
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int vaenmf_wiener(vaenmf_plan* p, const float* X2, const float* W, const float* Ht, const float* g,
                             const float* Zs, int32_t Rcap, int32_t R, const float* B1, const float* X,
                             float* S_hat, float* N_hat, float* WFs, float* WFn, void* stream) {
  if (int e = check_bound(p)) return e;
  if (int e = require_narrow(p, "vaenmf_wiener")) return e;
  VN_REQUIRE(R >= 1 && R <= Rcap, "bad R=%d (Rcap=%d)", R, Rcap);
  DecodeArgs a = base_decode_args(p, Zs, Rcap, R, B1);
  a.X2 = X2; a.W = W; a.Ht = const_cast<float*>(Ht); a.g = const_cast<float*>(g); a.X = X;
  a.S_hat = S_hat; a.N_hat = N_hat; a.WFs = WFs; a.WFn = WFn;
  { ProfScope ps(p, VN_K_WF, (hipStream_t)stream); launch_decode<MODE_WF>(p, a, (hipStream_t)stream); }
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

#ifdef VN_STAMP
extern "C" int vaenmf_debug_stamps(long long* out64, int reset) {
  long long h[64];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_stamp_store), sizeof(h)) != hipSuccess) return -2;
  for (int i = 0; i < 64; ++i) out64[i] = h[i];
  if (reset) { long long z[64] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_store), z, sizeof(z)); }
  return 0;
}
#endif
