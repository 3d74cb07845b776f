// Shared declarations for libvaenmf.so (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <type_traits>
#include <vector>
#include "../../include/vaenmf.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// ---- host side -------------------------------------------------------------
void vaenmf_set_error(const char* fmt, ...);
#define VN_CHECK_HIP(expr)                                                         \
  do {                                                                             \
    hipError_t _e = (expr);                                                        \
    if (_e != hipSuccess) {                                                        \
      vaenmf_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return -2;                                                                   \
    }                                                                              \
  } while (0)
#define VN_REQUIRE(cond, ...)                \
  do {                                       \
    if (!(cond)) {                           \
      vaenmf_set_error(__VA_ARGS__);         \
      return -1;                             \
    }                                        \
  } while (0)

constexpr int VN_COST_CHUNK = 25;     // EM iterations whose per-frame cost sums the fused driver keeps before one reduction launch
constexpr int MAX_TILE_FRAMES = 64;   // MH chain: frames per workgroup = 32 per team (2 MFMA column groups of 16)
constexpr int LAT = 32;               // latent dimension handled by the MFMA path
constexpr int HID = 128;              // hidden width of both decoder layers
constexpr int NK_H = HID / 32;        // k-steps over a hidden layer (4)
constexpr int NT_H = HID / 16;        // feature tiles of a hidden layer (8)
constexpr int VN_LDS_LIMIT = 160 * 1024;   // LDS of a CU: the most dynamic LDS a kernel is allowed (vn_ensure_dyn_lds)

// vaenmf_em_run as a HIP graph (driver.hip): the ~600 launches of a call captured once per call signature and replayed, so
// that the launch path needs the host once per call instead of once per kernel (a loaded host showed as up to 20 % of
// idle GPU time between the kernels)
struct VnEmGraphs {
  using Key = std::vector<uint64_t>;
  struct Graph {
    Key key; hipGraphExec_t exec; uint64_t used;
    int chain_kernel, w_fused;          // last_chain_kernel / last_w_fused as the captured body left them
  };
  hipStream_t cap_stream = nullptr;     // capture needs a stream of its own (the caller's may be the null stream)
  std::vector<Graph> cache;             // captured calls, a few signatures (a job alternates batch shapes: 63 / 62 utterances)
  std::vector<Key> seen;                // signatures run eagerly once (a signature is captured at its second appearance)
  uint64_t tick = 0;
  bool off = false;                     // capture failed once on this plan: stay eager
  int last = 0;                         // VAENMF_Q_EM_GRAPH: 1 when the last vaenmf_em_run was a graph launch
  Graph* find(const Key& key);                                          // a captured call of this signature, or null
  bool first_seen(const Key& key);                                      // true (and remembered) at a signature's first appearance
  Graph* insert(const Key& key, hipGraphExec_t exec, int chain_kernel, int w_fused);   // evicts the least recently used
  void release();                                                       // vaenmf_plan_destroy
};

// Where the sample-variance store keeps the row of (frame n, slot s) and its odd last bin F-1, in ELEMENTS of the store's
// type (bf16, or float in bf16x3 mode); every writer and reader of the store takes its addresses from here:
//   bins 0 .. of the row : n * frame + s * row
//   bin F-1              : xbase + n * xframe + s * xslot
// Padded layout (every F): a row is Fs elements with bin F-1 inside it (row = xslot = Fs, frame = xframe = Rs Fs,
// xbase = F-1).  F = 257 in bf16 is 544 B per row: every odd slot starts 32 B off a 64-byte block and every row shares
// its first and last cache line with its neighbours.
// Line-aligned layout (F = 256 c + 1, VAENMF_STORE_ALIGNED): a row is bins 0 .. 256 c - 1 and nothing else (512 c or
// 1024 c bytes), so every row starts on a 128-byte line and covers whole lines; bin F-1 of a frame's Rs slots is one
// contiguous block of Rs elements padded to 64 B, the blocks in a region of their own behind the rows of all frames.
struct VnStoreLayout {
  uint32_t row, frame;       // slot to slot, frame to frame
  uint32_t xslot, xframe;    // the same for bin F-1
  uint64_t xbase;            // bin F-1 of frame 0, slot 0
  int32_t aligned;           // 1: the line-aligned layout
};
// frames: frame blocks of the store (vaenmf_mh_chain: NT + 1, a spare block for lanes without a frame); esz: 2 or 4
inline VnStoreLayout vn_store_layout_of(int F, int Fs, int esz, int Rs, size_t frames, bool aligned) {
  VnStoreLayout l;
  if (aligned && (F == 257 || F == 513)) {
    l.row = (uint32_t)(F - 1); l.frame = (uint32_t)Rs * l.row;
    l.xslot = 1; l.xframe = (uint32_t)(((size_t)Rs * esz + 63) / 64 * 64 / esz);
    l.xbase = (uint64_t)frames * l.frame; l.aligned = 1;
  } else {
    l.row = l.xslot = (uint32_t)Fs; l.frame = l.xframe = (uint32_t)Rs * (uint32_t)Fs;
    l.xbase = (uint64_t)(F - 1); l.aligned = 0;
  }
  return l;
}
// bytes of a store of `frames` frame blocks (both regions)
inline size_t vn_store_bytes(const VnStoreLayout& l, size_t frames, int esz) {
  return (l.aligned ? frames * ((size_t)l.frame + l.xframe) : frames * (size_t)l.frame) * esz;
}

struct vaenmf_plan {
  vaenmf_config cfg;
  int Fs, Kp, NT3;           // padded bins, padded rank, feature tiles of 16 on the MFMA path of the last layer
  int Fm;                    // bins on the MFMA path: F-1 when F = 16k+1 (the odd last bin is computed in fp32 FMA), else F
  float* w3n;                // [HID] fp32 row F-1 of the last layer (odd last bin)
  int geom;                  // workgroup geometry (engine.hip: with_geom)
  int nwaves;                // waves of a team that split the features
  int tile_frames;           // MH-chain frames per workgroup: 64 (2 teams of 4 waves) or 32 (1 team of 8)
  // decoder weights on the device, MFMA fragment order (see weights in plan.hip)
  __bf16 *w1f, *w2f, *w3f;   // [tile][kstep][part hi/lo][lane][8]
  float *b1, *b2, *b3;       // biases (b3 padded to 16*NT3)
  float* w1y;                // [H1][Dy] label columns of W1 (M2)
  int Dy;
  int Lz;                    // latent dimension of the model: latents Lz..Lp-1 of the MFMA path are zero padding
  bool wide = false;         // L > 32 or H1 = 256: the chain is wide.hip's kernel, M-step and Wiener filter stream the store
  int Lp = LAT;              // latent columns of Z / Zs / the replay draws: 32, or 128 on a wide plan (VAENMF_Q_LP)
  bool one_hidden;           // decoder with ONE hidden layer (h_dim = [128]): layer 2 is skipped
  bool have_weights;
  const float* Vb_ext;       // caller-owned noise variance [NT][Fs] (noNMF variants) or null
  // bound batch
  int n_utt, NT, n_tiles;
  int32_t *d_frame_off;      // [n_utt+1]
  int32_t *d_tile_utt, *d_tile_n0, *d_tile_cnt;   // MH-chain tiles (<=32 frames, one utterance each)
  int32_t *d_frame_utt;      // [NT]
  int32_t *d_frame_loc;      // [NT] frame index inside its utterance
  // wave-private chain (chain.hip): all F bins on the MFMA path, W3 / b3 in the chain's bin order; wave tiles
  __bf16* w3c;               // [NT3c][kstep][part][lane][8]
  float* b3c;                // [16 NT3c], padding -200
  int NT3c;                  // ceil(F / 16)
  int32_t *d_wt_utt, *d_wt_n0, *d_wt_cnt;         // wave tiles (<= 16 frames of one utterance each)
  int n_wtiles;
  // tiles of <= 64 consecutive frames of one utterance (wstats_fused_kernel: one workgroup per tile) and the partial sums of
  // the W update, one [Fs][2 Kp] block per tile
  int32_t *d_t64_n0 = nullptr, *d_t64_cnt = nullptr, *d_t64_first = nullptr, *d_t64_g0 = nullptr;      // [n_t64], [n_t64], [n_utt+1]
  int n_t64 = 0;
  float* wpart64 = nullptr;
  size_t wpart16_groups = 0; // capacity of wpart16 in 16-frame groups
  float* wpart16 = nullptr;  // [n_sms][2 Kp][Fs]: per-16-frame-group partials of wstats_group_kernel (small batches, rank <= 8)
  int last_chain_kernel = 0; // VAENMF_Q_CHAIN_KERNEL
  int last_w_fused = 0;      // VAENMF_Q_W_FUSED: 1 when the last stored M-step ran the fused W-statistics kernel
  int Rcap_store;            // samples per frame the store was sized for at vaenmf_bind_batch / vaenmf_sample_store
  int last_m_step_path;      // VAENMF_Q_MSTEP_PATH: 0 none yet, 1 stored (streaming), 2 decoding
  uint64_t* d_utt_seed;      // [n_utt]
  std::vector<int32_t> h_frame_off;
  // workspace
  float *A1, *P;             // [NT][Fs] W-update statistics
  float* normW;              // [n_utt][Kp]
  float* wpart;              // [n_utt][8 chunks][Fs][2 Kp] partial W-update sums
  double* cost_frames;       // [VN_COST_CHUNK][max_frames] per-frame cost sums of the fused driver (a row per iteration of a chunk)
  // sample-variance store (vaenmf_sample_store): the MH chain keeps the decoded variances of its samples here
  bool store_on;
  void* VsS;                 // [NT + 1] frame blocks of store_Rs rows, float (bf16x3 mode) or bf16 (bf16 mode), laid out as store_lay
  int32_t* src;              // [NT][store_Rs]
  size_t VsS_cap, src_cap;   // allocated bytes / elements
  int store_R, store_Rs;     // samples / slots per frame of the last chain that filled the store (0: empty)
  VnStoreLayout store_lay;   // ... and the layout it wrote them in
  int n_sms;
  // optional per-kernel timing with HIP events on the launch stream (vaenmf_profile_*)
  bool prof_on;
  std::vector<hipEvent_t> prof_ev;      // pairs (start, stop)
  std::vector<int> prof_kind;
  size_t prof_used;
  VnEmGraphs graphs;
  // vaenmf_bind_batch_async: the per-batch seeds go up from a ring of pinned slots (a slot is reused when its copy is done)
  static constexpr int SEED_RING = 8;
  uint64_t* h_seed_ring = nullptr;      // pinned [SEED_RING][max_utts]
  hipEvent_t seed_ev[SEED_RING] = {};
  bool seed_ev_used[SEED_RING] = {};
  int seed_pos = 0;
};

// one MH-chain call, as vaenmf_mh_chain hands it to the kernel launchers (engine.hip team kernel, chain.hip wave kernel,
// wide.hip wide kernel)
struct VnChainCall {
  const float *X2, *W, *Ht, *g, *B1;
  float *Z, *Zs, *acc_out;
  const float *eps, *u;
  void* VsS; size_t VsS_bytes; int32_t* src; int Rs;
  VnStoreLayout lay;         // of the store for this call's Rs (vn_store_layout)
  int Rcap, nsamples, burnin, rng_mode, update_Z;
  uint32_t call;
  float sd;
  float sd_hi;               // random-walk step of latents 16..31: sd, or 0 when they are padding (latent dimension 16)
  int one_hidden;
};

// Kernel-choice switches for tests and A/B runs, read from the environment on every call (tests change them inside one
// process); vaenmf_em_run keys its graphs on them.  plan.hip
struct VnSwitches {
  bool wchain4;        // VAENMF_WCHAIN4=0: small batches stay on wchain_kernel instead of wchain4_kernel
  bool team_chain;     // VAENMF_TEAM_CHAIN=1: the team kernel of engine.hip for every shape
  bool wfused;         // VAENMF_WFUSED=0: W statistics + W update as two kernels
  bool wgroup;         // VAENMF_WGROUP=0: small batches stay on wstats_fused_kernel instead of wstats_group_kernel
  int wfused_grid;     // VAENMF_WFUSED_GRID=n: at most n workgroups for wstats_fused_kernel (0: no cap)
  int grid_cap;        // VAENMF_GRID_CAP=n: at most n workgroups for the persistent kernels -- wchain_kernel, decode_kernel, the streaming
                       // kernels of stream.hip -- so that a small batch walks their tile / frame loops several times (tests; 0: no cap)
  bool keep_zs;        // VAENMF_KEEP_ZS=1: the E-step chains of the sample-store path record their samples anyway
  bool store_aligned;  // VAENMF_STORE_ALIGNED=0: the padded store layout for every F (VnStoreLayout)
};

// ---- functions one source file defines and another calls (the file that defines each) ----
VnSwitches vn_switches();                                  // plan.hip
int vn_ensure_dyn_lds(const void* fn, int bytes);          // plan.hip: per-device hipFuncSetAttribute, checked
extern long long g_vn_dev_allocs;                          // plan.hip: device allocations made by the library (VAENMF_Q_DEV_ALLOCS)
bool vn_wchain_supported(const vaenmf_plan* p);            // chain.hip
bool vn_wchain_fits(const vaenmf_plan* p, const VnChainCall& cc);                 // chain.hip
bool vn_wchain_park_fits(const vaenmf_plan* p, int Rs, bool m2);                  // chain.hip: LDS for the odd bins of Rs slots beside the weights
VnStoreLayout vn_store_layout(const vaenmf_plan* p, int Rs, bool m2);             // driver.hip: the store's layout for chains of Rs slots (m2: with B1)
int vn_launch_wchain(vaenmf_plan* p, const VnChainCall& cc, hipStream_t st);      // chain.hip: builds WcArgs, picks the kernel
int vn_launch_tchain(vaenmf_plan* p, const VnChainCall& cc, hipStream_t st);      // engine.hip: builds ChainArgs, picks the geometry
int vn_launch_widechain(vaenmf_plan* p, const VnChainCall& cc, hipStream_t st);   // wide.hip: the chain of a wide plan
int vn_launch_wide_rng_fill(vaenmf_plan* p, uint32_t call, int S, float* eps_out, float* u_out, hipStream_t st);   // engine.hip: rng_fill_kernel over the wave tiles
int vn_launch_w_update(const vaenmf_plan* p, float* W, const float* Ht, hipStream_t st);                // aux.hip
int vn_launch_w_update_tiles(const vaenmf_plan* p, float* W, hipStream_t st, bool groups);             // aux.hip
int vn_launch_cost_reduce(const vaenmf_plan* p, const double* cost_frames, size_t stride, int n_it, int R, double* cost, int niter,
                          int it0, hipStream_t st);                                                     // aux.hip

inline int check_bound(const vaenmf_plan* p) {
  VN_REQUIRE(p != nullptr, "null plan");
  VN_REQUIRE(p->have_weights, "decoder weights not set (vaenmf_set_decoder_weights)");
  VN_REQUIRE(p->NT > 0, "no batch bound (vaenmf_bind_batch)");
  return 0;
}

enum { VN_K_CHAIN = 0, VN_K_WSTATS = 1, VN_K_WUPDATE = 2, VN_K_HG = 3, VN_K_WF = 4, VN_K_NKINDS = 5 };
struct ProfScope {   // records a (start, stop) event pair around a launch when profiling is on
  vaenmf_plan* p; hipStream_t st; size_t idx; bool on;
  ProfScope(vaenmf_plan* p_, int kind, hipStream_t st_) : p(p_), st(st_), idx(0), on(false) {
    if (p && p->prof_on && p->prof_used + 2 <= p->prof_ev.size()) {
      on = true; idx = p->prof_used; p->prof_used += 2; p->prof_kind[idx / 2] = kind;
      (void)hipEventRecord(p->prof_ev[idx], st);
    }
  }
  ~ProfScope() { if (on) (void)hipEventRecord(p->prof_ev[idx + 1], st); }
};

// ---- device helpers --------------------------------------------------------
#if defined(__HIPCC__)
// The decoder weights are pre-scaled on the host (plan.hip): hidden layers by 2 log2(e), the output layer by
// log2(e), so the MFMA accumulators are already the arguments of v_exp_f32 (2^x):
//   tanh(x) = 1 - 2/(exp(2x)+1) = 1 - 2/(2^(xs)+1),  xs = 2 log2(e) x      (abs error ~2e-7)
//   exp(a)  = 2^(as),                                 as = log2(e) a
__device__ __forceinline__ float fast_tanh(float xs) {
  float e = __builtin_amdgcn_exp2f(xs);
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}
__device__ __forceinline__ float fast_exp(float as) { return __builtin_amdgcn_exp2f(as); }
__device__ __forceinline__ float fast_log(float x) { return __builtin_amdgcn_logf(x) * 0.6931471805599453f; }
__device__ __forceinline__ float fast_log2(float x) { return __builtin_amdgcn_logf(x); }
constexpr float LN2_F = 0.6931471805599453f;
__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }

// split 4 floats into bf16 hi and lo parts: v ~= hi + lo (error ~2^-17 |v|)
__device__ __forceinline__ void split4(const f32x4 v, bf16x4& hi, bf16x4& lo) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    __bf16 h = (__bf16)v[t];
    hi[t] = h;
    lo[t] = (__bf16)(v[t] - (float)h);
  }
}

// 8 floats -> the bf16 (hi, lo) parts of one MFMA operand (lo is zero in bf16 mode)
template <bool SPLIT>
__device__ __forceinline__ void split8(const float (&z)[8], bf16x8& hi, bf16x8& lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    __bf16 h = (__bf16)z[j];
    hi[j] = h;
    lo[j] = SPLIT ? (__bf16)(z[j] - (float)h) : (__bf16)0.f;
  }
}

// ---- fragment blocks [part hi/lo][lane][8 bf16] of the team and wide kernels (engine.hip's header has the order) ----
// this lane's MFMA operand of the block at p (p includes lane16 = 16 * lane): the lo part sits 1024 bytes behind the hi
// part in bf16x3 mode; bf16 mode has none (and mma3 reads none)
template <bool SPLIT>
__device__ __forceinline__ void load_frag(const char* p, bf16x8& hi, bf16x8& lo) {
  hi = *reinterpret_cast<const bf16x8*>(p);
  if (SPLIT) lo = *reinterpret_cast<const bf16x8*>(p + 1024); else lo = hi;
}
// tanh, split and store feature tile t of a layer into the activation image [k-step][part][lane][8 bf16] of one column
// group: tile t is half (t & 1) of k-step t >> 1.  Returns the tanh values.
template <bool SPLIT>
__device__ __forceinline__ f32x4 store_act_tile(char* img, unsigned lane16, int t, const f32x4 acc) {
  f32x4 h;
#pragma unroll
  for (int k = 0; k < 4; ++k) h[k] = fast_tanh(acc[k]);
  bf16x4 hi, lo;
  split4(h, hi, lo);
  char* p = img + (t >> 1) * (SPLIT ? 2 : 1) * 1024 + lane16 + (t & 1) * 8;
  *reinterpret_cast<bf16x4*>(p) = hi;
  if (SPLIT) *reinterpret_cast<bf16x4*>(p + 1024) = lo;
  return h;
}

// a latent row in fragment order: eight floats <-> the quads at row + o0 and row + o1 (team kernels: latents 4q.. and
// 16 + 4q..; wide kernel: the same inside k-step w)
__device__ __forceinline__ void load_row8(const float* row, int o0, int o1, float (&z)[8]) {
  const f32x4 lo = *reinterpret_cast<const f32x4*>(row + o0);
  const f32x4 hi = *reinterpret_cast<const f32x4*>(row + o1);
#pragma unroll
  for (int t = 0; t < 4; ++t) { z[t] = lo[t]; z[4 + t] = hi[t]; }
}
__device__ __forceinline__ void store_row8(float* row, int o0, int o1, const float (&z)[8]) {
  *reinterpret_cast<f32x4*>(row + o0) = f32x4{z[0], z[1], z[2], z[3]};
  *reinterpret_cast<f32x4*>(row + o1) = f32x4{z[4], z[5], z[6], z[7]};
}

// (widechain_kernel; mh_chain_kernel keeps the same lines written out)
// Per-(bin, frame) constants of a chain in accumulator layout, for the bins f0 .. f0 + 3 of one frame: X2, and Vb = W H
// (mcem.py:81-82) or the plan's fixed Vb [NT][Fs] (non-null).  X2 [NT][Fs], W [utt][Fs][Kp], Ht [NT][Kp]; n: the frame's row, utt: its utterance.  A tile the
// wavefront does not own (!own) and the padding bins (>= F_end) get X2 = 0, Vb = 1; with Vs = 0 there (zero W3 rows, a
// large negative bias) their energy term is exactly 0.
__device__ __forceinline__ void tile_consts4(bool own, const float* X2, const float* Vb, const float* W, const float* Ht, int Fs, int Kp,
                                             int n, int utt, int f0, int F_end, f32x4& x2, f32x4& vb) {
  f32x4 xv = {0, 0, 0, 0}, v = {0, 0, 0, 0};
  if (own) {
    xv = *reinterpret_cast<const f32x4*>(X2 + (size_t)n * Fs + f0);
    if (Vb) {
      v = *reinterpret_cast<const f32x4*>(Vb + (size_t)n * Fs + f0);
    } else {
      for (int k = 0; k < Kp; k += 4) {
        const f32x4 h = *reinterpret_cast<const f32x4*>(Ht + (size_t)n * Kp + k);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const f32x4 wr = *reinterpret_cast<const f32x4*>(W + ((size_t)utt * Fs + f0 + t) * Kp + k);
          v[t] += wr[0] * h[0] + wr[1] * h[1] + wr[2] * h[2] + wr[3] * h[3];
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (f0 + t >= F_end) { xv[t] = 0.f; v[t] = 1.f; }
  x2 = xv;
  vb = v;
}

// one MFMA step of a decoder layer: bf16x3 (SPLIT) adds the two cross terms of the (hi, lo) parts
template <bool SPLIT>
__device__ __forceinline__ f32x4 mma3(const bf16x8 whi, const bf16x8 wlo, const bf16x8 ahi, const bf16x8 alo, f32x4 acc) {
  // weights are the A operand (rows = output features), activations the B operand
  if (SPLIT) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wlo, ahi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(whi, alo, acc, 0, 0, 0);
  }
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(whi, ahi, acc, 0, 0, 0);
}

// ---- cross-lane sums without LDS traffic (DPP / permlane-swap VALU ops) ----------------
// lane = 16 q + c: sum over c (the 16 lanes of a DPP row), over q (the 4 rows), or over the wave
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float sum_row16(float v) {       // every lane gets the sum over its row
  v += dpp_mov<0xB1>(v);     // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);     // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);    // row_half_mirror
  v += dpp_mov<0x140>(v);    // row_mirror
  return v;
}
// v_permlane{16,32}_swap exchange halves between TWO registers; feeding one value twice lets
// the compiler assign both operands the same register (a no-op swap), so the copy is made opaque.
__device__ __forceinline__ unsigned opaque_copy(unsigned a) {
  unsigned b = a;
  asm volatile("" : "+v"(b));
  return b;
}
__device__ __forceinline__ float swap16_add(float v) {      // v[l] + v[l ^ 16]
  const unsigned a = __builtin_bit_cast(unsigned, v);
  auto r = __builtin_amdgcn_permlane16_swap(a, opaque_copy(a), false, false);
  unsigned x = r[0], y = r[1];
  asm volatile("" : "+v"(x), "+v"(y));      // keep both halves of the result (hipcc 7.2 folds r[1] into r[0] otherwise)
  return __builtin_bit_cast(float, x) + __builtin_bit_cast(float, y);
}
__device__ __forceinline__ float swap32_add(float v) {      // v[l] + v[l ^ 32]
  const unsigned a = __builtin_bit_cast(unsigned, v);
  auto r = __builtin_amdgcn_permlane32_swap(a, opaque_copy(a), false, false);
  unsigned x = r[0], y = r[1];
  asm volatile("" : "+v"(x), "+v"(y));
  return __builtin_bit_cast(float, x) + __builtin_bit_cast(float, y);
}
__device__ __forceinline__ float sum_rows4(float v) { return swap32_add(swap16_add(v)); }   // sum over q
// Several sums over q at once: the swaps are fed two DIFFERENT values, so neither half of an exchange is thrown away and no
// opaque copy is needed.  With r0..r3 the four rows of a register,
//   v_permlane16_swap(a, b) leaves [a0 b0 a2 b2] and [a1 b1 a3 b3]; their sum is [a0+a1, b0+b1, a2+a3, b2+b3]
//   v_permlane32_swap(s, t) leaves [s0 s1 t0 t1] and [s2 s3 t2 t3]; their sum is [s0+s2, s1+s3, t0+t2, t1+t3]
// Every total is (r0 + r1) + (r2 + r3), the tree of sum_rows4: the same bits.
__device__ __forceinline__ float swap16_add2(float a, float b) {
  auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b), false, false);
  unsigned x = r[0], y = r[1];
  asm volatile("" : "+v"(x), "+v"(y));      // (as in swap16_add: r[0] + r[0] is emitted otherwise, with different operands too)
  return __builtin_bit_cast(float, x) + __builtin_bit_cast(float, y);
}
__device__ __forceinline__ float swap32_add2(float s, float t) {
  auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, s), __builtin_bit_cast(unsigned, t), false, false);
  unsigned x = r[0], y = r[1];
  asm volatile("" : "+v"(x), "+v"(y));
  return __builtin_bit_cast(float, x) + __builtin_bit_cast(float, y);
}
// rows 0 and 2 (lanes 0-15, 32-47) hold the sum over q of a, rows 1 and 3 (lanes 16-31, 48-63) that of b
__device__ __forceinline__ float sum_rows4_x2(float a, float b) { return swap32_add(swap16_add2(a, b)); }
// row j (lanes 16 j .. 16 j + 15) holds the sum over q of the j-th argument
__device__ __forceinline__ float sum_rows4_x4(float a, float b, float c, float d) {
  return swap32_add2(swap16_add2(a, b), swap16_add2(c, d));
}
__device__ __forceinline__ double swap16_add_d(double v) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)b, hi = (unsigned)(b >> 32);
  auto rl = __builtin_amdgcn_permlane16_swap(lo, opaque_copy(lo), false, false);
  auto rh = __builtin_amdgcn_permlane16_swap(hi, opaque_copy(hi), false, false);
  const double a0 = __builtin_bit_cast(double, ((unsigned long long)rh[0] << 32) | rl[0]);
  const double a1 = __builtin_bit_cast(double, ((unsigned long long)rh[1] << 32) | rl[1]);
  return a0 + a1;
}
__device__ __forceinline__ double swap32_add_d(double v) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)b, hi = (unsigned)(b >> 32);
  auto rl = __builtin_amdgcn_permlane32_swap(lo, opaque_copy(lo), false, false);
  auto rh = __builtin_amdgcn_permlane32_swap(hi, opaque_copy(hi), false, false);
  const double a0 = __builtin_bit_cast(double, ((unsigned long long)rh[0] << 32) | rl[0]);
  const double a1 = __builtin_bit_cast(double, ((unsigned long long)rh[1] << 32) | rl[1]);
  return a0 + a1;
}
__device__ __forceinline__ double sum_rows4_d(double v) { return swap32_add_d(swap16_add_d(v)); }

// ---- radix-2 FFT in LDS, fp64 (fft.hip: STFT / iSTFT and the Bluestein convolution; stoi.hip: band spectra) ----
__device__ __forceinline__ int bitrev(int x, int bits) { return (int)(__brev((unsigned)x) >> (32 - bits)); }

// in-place complex FFT of length n (power of two) on LDS arrays whose input is in bit-reversed order; the whole workgroup
// calls it; the twiddle of step t is twr[t] + i sign twi[t] (t < n / 2)
__device__ inline void fft_lds(double* re, double* im, const double* twr, const double* twi, int n, int bits, int sign) {
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

// xoshiro128+ : per-lane stream, 32 random bits per call, no multiplies
struct Xs128 {
  uint32_t s0, s1, s2, s3;
  __device__ __forceinline__ uint32_t next() {
    uint32_t r = s0 + s3;
    uint32_t t = s1 << 9;
    s2 ^= s0; s3 ^= s1; s1 ^= s2; s0 ^= s3; s2 ^= t;
    s3 = (s3 << 11) | (s3 >> 21);
    return r;
  }
};
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t& x) {
  uint64_t z = (x += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// stream key: (utterance seed, frame index inside the utterance, sub-stream id, chain call)
__device__ __forceinline__ Xs128 xs_seed(uint64_t utt_seed, uint32_t frame, uint32_t sub, uint32_t call) {
  uint64_t x = utt_seed ^ (((uint64_t)frame << 32) | ((uint64_t)sub << 24) | (uint64_t)(call & 0xFFFFFFu));
  x ^= (uint64_t)(call >> 24) << 56;
  uint64_t a = splitmix64(x), b = splitmix64(x);
  Xs128 s;
  s.s0 = (uint32_t)a; s.s1 = (uint32_t)(a >> 32); s.s2 = (uint32_t)b; s.s3 = (uint32_t)(b >> 32);
  if ((s.s0 | s.s1 | s.s2 | s.s3) == 0) s.s0 = 1;
  return s;
}
// 4 standard normals (two Box-Muller pairs); v_sin/v_cos take revolutions.
// ONE random word per pair -- radius from its high 16 bits, angle from its low 16 bits -- instead of two
// words at 24 bits each: half the generator steps (the proposals are N(0, var_RW) steps of a random walk: a radius on a
// 2^-16 grid, |eps| <= 4.71 sigma, changes nothing the sampler's distribution can show; any symmetric proposal leaves
// the Metropolis-Hastings target unchanged).
__device__ __forceinline__ f32x4 normal4(Xs128& st) {
  f32x4 o;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const uint32_t a = st.next();
    const float u1 = ((float)(a >> 16) + 1.0f) * 1.52587890625e-5f;  // (0,1], 2^-16 grid
    const float u2 = (float)(a & 0xFFFFu) * 1.52587890625e-5f;       // [0,1)
    float r = __builtin_amdgcn_sqrtf(-2.0f * fast_log(u1));
    o[2 * p] = r * __builtin_amdgcn_cosf(u2);
    o[2 * p + 1] = r * __builtin_amdgcn_sinf(u2);
  }
  return o;
}
__device__ __forceinline__ float uniform01(Xs128& st) { return (float)(st.next() >> 8) * 5.9604644775390625e-8f; }

// ---- pass schedule of an MH chain (every chain kernel: chain.hip, engine.hip, wide.hip) ----
// Pass it = -1 evaluates the initial state (mcem.py:392-400); the MH steps m = 0 .. burnin + nsamples - 1 follow.  With the
// sample-variance store on (STORE) and a burn-in, one more pass right after the burn-in (`re`) evaluates the state the
// chain is in again -- nothing drawn, nothing decided -- so that its variances are on record.
// The store's contract, as stream.hip, vaenmf_sample_store_gather and the oracle read it: a pass writes the variances of
// the state it evaluates to `slot` (-1: none).  Slot r < nsamples holds the proposal of post-burn-in step r; slot nsamples
// holds the state the chain is in when the burn-in ends (the initial state when there is no burn-in).
struct VnChainPass {
  bool re;       // the re-evaluation pass
  int m;         // MH step of the pass (-1: the initial state; on the re-evaluation pass: burnin, not taken)
  bool step;     // an MH step: noise is drawn, the proposal decided
  int slot;
};
template <bool STORE>
__device__ __forceinline__ int vn_chain_passes(int nsamples, int burnin) {      // the loop is for (it = -1; it < passes; ++it)
  return nsamples + burnin + ((STORE && burnin > 0) ? 1 : 0);
}
template <bool STORE>
__device__ __forceinline__ VnChainPass vn_chain_pass(int it, int nsamples, int burnin) {
  const bool reeval = STORE && burnin > 0;
  VnChainPass p;
  p.re = reeval && it == burnin;
  p.m = (reeval && it > burnin) ? it - 1 : it;
  p.step = p.m >= 0 && !p.re;
  p.slot = !STORE ? -1 : (p.re ? nsamples : (p.m >= burnin ? p.m - burnin : ((p.m < 0 && burnin == 0) ? nsamples : -1)));
  return p;
}
#endif
