// Host driver of the library: the entry points that orchestrate more than one launch.  vaenmf_mh_chain chooses between the
// wave-private chain kernels (chain.hip) and the team kernel (engine.hip) and checks the sample-variance store;
// vaenmf_sample_store sizes that store; vaenmf_em_run runs a whole reconstruct call, as a replayed HIP graph from a call
// signature's second appearance on.  The only device code here is the store's gather kernel.
#include "common.h"
#include <cstring>

// The layout the chains of Rs slots write the store in and its readers read it in (VnStoreLayout, common.h): line-aligned
// for F = 257 / 513 unless VAENMF_STORE_ALIGNED=0 -- or unless the wave-private chain kernels, which collect a frame's odd
// bins in LDS, have no room for Rs of them beside their weights (vn_wchain_park_fits)
VnStoreLayout vn_store_layout(const vaenmf_plan* p, int Rs, bool m2) {
  const int esz = p->cfg.precision == VAENMF_PREC_BF16X3 ? 4 : 2;
  bool aligned = vn_switches().store_aligned;
  if (aligned && !p->wide && vn_wchain_supported(p) && !vn_wchain_park_fits(p, Rs, m2)) aligned = false;
  return vn_store_layout_of(p->cfg.F, p->Fs, esz, Rs, (size_t)(p->NT > 0 ? p->NT : p->cfg.max_frames) + 1, aligned);
}
extern "C" int vaenmf_store_layout(int32_t F, int32_t Fs, int32_t elt_bytes, int32_t Rs, int64_t frames, int32_t aligned, int64_t* out7) {
  VN_REQUIRE(out7 != nullptr && F >= 1 && Fs >= F && (elt_bytes == 2 || elt_bytes == 4) && Rs >= 1 && frames >= 1, "vaenmf_store_layout: bad arguments");
  const VnStoreLayout l = vn_store_layout_of(F, Fs, elt_bytes, Rs, (size_t)frames, aligned != 0);
  out7[0] = l.row; out7[1] = l.frame; out7[2] = l.xslot; out7[3] = l.xframe; out7[4] = (int64_t)l.xbase; out7[5] = l.aligned;
  out7[6] = (int64_t)vn_store_bytes(l, (size_t)frames, elt_bytes);
  return 0;
}

extern "C" int vaenmf_mh_chain(vaenmf_plan* p, const float* X2, const float* W, const float* Ht, const float* g,
                               float* Z, int32_t update_Z, const float* B1, float* Zs, int32_t Rcap, int32_t nsamples,
                               int32_t burnin, float var_rw, const vaenmf_rng* rng, float* acc_out, void* stream) {
  if (int e = check_bound(p)) return e;
  VN_REQUIRE(rng != nullptr, "rng is null");
  VN_REQUIRE(nsamples >= 1 && burnin >= 0 && nsamples <= Rcap, "bad sample counts (nsamples=%d burnin=%d Rcap=%d)", nsamples, burnin, Rcap);
  VN_REQUIRE(rng->mode == VAENMF_RNG_DEVICE || (rng->eps && rng->u), "replay mode needs eps and u buffers");
  hipStream_t st = (hipStream_t)stream;
  const bool split = p->cfg.precision == VAENMF_PREC_BF16X3;
  VnChainCall cc = {};
  cc.X2 = X2; cc.W = W; cc.Ht = Ht; cc.g = g; cc.B1 = B1; cc.Z = Z; cc.Zs = Zs; cc.acc_out = acc_out;
  cc.eps = rng->eps; cc.u = rng->u;
  cc.Rcap = Rcap; cc.nsamples = nsamples; cc.burnin = burnin; cc.rng_mode = rng->mode; cc.update_Z = update_Z;
  cc.call = rng->call; cc.sd = sqrtf(var_rw); cc.sd_hi = p->Lz > 16 ? cc.sd : 0.f; cc.one_hidden = p->one_hidden ? 1 : 0;
  p->store_R = p->store_Rs = 0;
  if (p->store_on) {                                    // sample-variance store: sized by vaenmf_sample_store, never here
    const int Rs = nsamples + 1;
    const VnStoreLayout lay = vn_store_layout(p, Rs, B1 != nullptr);
    const size_t need_v = vn_store_bytes(lay, (size_t)p->NT + 1, split ? 4 : 2), need_s = (size_t)p->NT * Rs;   // + a spare block (idle lanes); rows and odd bins
    VN_REQUIRE(need_v < 0xE0000000ull, "sample store: %d frames x %d slots x %d bins exceeds the 32-bit byte offsets of "
               "the chain kernel; bind a smaller batch or switch the store off", p->NT, Rs, p->Fs);
    VN_REQUIRE(need_v <= p->VsS_cap && need_s <= p->src_cap, "sample store too small for %d frames x %d samples: call "
               "vaenmf_sample_store(plan, max_samples) after vaenmf_bind_batch (no allocation happens in vaenmf_mh_chain)", p->NT, nsamples);
    cc.VsS = p->VsS; cc.VsS_bytes = need_v; cc.src = p->src; cc.Rs = Rs; cc.lay = lay;
  }
  // wide decoder shapes: one kernel for every batch (wide.hip, 64-bit addresses).  Else wave-private chains (chain.hip)
  // while every buffer of the batch is within their 32-bit byte offsets; a larger batch (about 300 k frames at 105
  // samples) runs engine.hip's team kernel, which addresses with 64 bits
  const bool use_wchain = !p->wide && vn_wchain_supported(p) && vn_wchain_fits(p, cc);
  VN_REQUIRE(p->wide || use_wchain || Zs != nullptr, "vaenmf_mh_chain: Zs may be NULL only where the wave-private chain kernels run (vaenmf_wchain_addressable)");
  {                                                     // each launcher records its kernel in last_chain_kernel
    ProfScope ps(p, VN_K_CHAIN, st);
    if (int e = p->wide ? vn_launch_widechain(p, cc, st) : use_wchain ? vn_launch_wchain(p, cc, st) : vn_launch_tchain(p, cc, st)) return e;
  }
  if (p->store_on) { p->store_R = nsamples; p->store_Rs = nsamples + 1; p->store_lay = cc.lay; }
  return 0;
}

// max_samples > 0: switch the store on and size it for chains of up to max_samples samples per frame over the
// plan's frame capacity (an allocating call, like vaenmf_plan_create); 0: off (the memory is kept).
extern "C" int vaenmf_sample_store(vaenmf_plan* p, int32_t max_samples) {
  VN_REQUIRE(p != nullptr, "null plan");
  VN_REQUIRE(max_samples >= 0, "max_samples = %d", max_samples);
  p->store_R = p->store_Rs = 0;
  p->store_on = max_samples > 0;
  if (!p->store_on) return 0;
  const size_t esz = p->cfg.precision == VAENMF_PREC_BF16X3 ? sizeof(float) : sizeof(__bf16);
  // sized for the bound batch (or, before a batch is bound, for the plan's frame capacity)
  const size_t frames = (size_t)(p->NT > 0 ? p->NT : p->cfg.max_frames) + 1, Rs = (size_t)max_samples + 1;
  // (both layouts: VAENMF_STORE_ALIGNED is read at every chain call)
  const size_t need_pad = vn_store_bytes(vn_store_layout_of(p->cfg.F, p->Fs, (int)esz, (int)Rs, frames, false), frames, (int)esz);
  const size_t need_aln = vn_store_bytes(vn_store_layout_of(p->cfg.F, p->Fs, (int)esz, (int)Rs, frames, true), frames, (int)esz);
  size_t need_v = need_pad > need_aln ? need_pad : need_aln, need_s = frames * Rs;
  if (need_v >= 0xE0000000ull) need_v = 0xE0000000ull - 16;    // larger batches fall back to decoding (vaenmf_em_run); offsets from 0xF0000000 mark idle lanes
  if (need_v > p->VsS_cap) {
    if (p->VsS) VN_CHECK_HIP(hipFree(p->VsS));
    p->VsS = nullptr; p->VsS_cap = 0;
    VN_CHECK_HIP(hipMalloc(&p->VsS, need_v));
    ++g_vn_dev_allocs;
    p->VsS_cap = need_v;
  }
  if (need_s > p->src_cap) {
    if (p->src) VN_CHECK_HIP(hipFree(p->src));
    p->src = nullptr; p->src_cap = 0;
    VN_CHECK_HIP(hipMalloc(&p->src, need_s * sizeof(int32_t)));
    ++g_vn_dev_allocs;
    p->src_cap = need_s;
  }
  p->Rcap_store = max_samples;
  return 0;
}

namespace {
// (line-aligned layout: the row's bins, bin F-1 from the frame's block of odd bins, zeros in the padding)
template <typename ST>
__global__ void store_gather_kernel(const ST* __restrict__ VsS, const int32_t* __restrict__ src, int NT, int R, VnStoreLayout lay, int F, int Fs,
                                    float* __restrict__ out) {
  const int n = blockIdx.x / R, r = blockIdx.x - n * R;
  const int sl = src[(size_t)r * NT + n];
  const ST* row = VsS + (size_t)n * lay.frame + (size_t)sl * lay.row;
  const ST* xp = VsS + lay.xbase + (size_t)n * lay.xframe + (size_t)sl * lay.xslot;
  for (int f = threadIdx.x; f < Fs; f += blockDim.x)
    out[((size_t)n * R + r) * Fs + f] = f < (int)lay.row ? (float)row[f] : (f == F - 1 ? (float)*xp : 0.f);
}
}  // namespace

extern "C" int vaenmf_sample_store_gather(vaenmf_plan* p, float* Vs_out, void* stream) {
  VN_REQUIRE(p != nullptr && p->store_R > 0, "the sample store is empty (vaenmf_sample_store(plan, 1), then vaenmf_mh_chain)");
  VN_REQUIRE(Vs_out != nullptr, "null output");
  if (p->cfg.precision == VAENMF_PREC_BF16X3)
    hipLaunchKernelGGL(store_gather_kernel<float>, dim3((unsigned)(p->NT * p->store_R)), dim3(64), 0, (hipStream_t)stream,
                       reinterpret_cast<const float*>(p->VsS), p->src, p->NT, p->store_R, p->store_lay, p->cfg.F, p->Fs, Vs_out);
  else
    hipLaunchKernelGGL(store_gather_kernel<__bf16>, dim3((unsigned)(p->NT * p->store_R)), dim3(64), 0, (hipStream_t)stream,
                       reinterpret_cast<const __bf16*>(p->VsS), p->src, p->NT, p->store_R, p->store_lay, p->cfg.F, p->Fs, Vs_out);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int vaenmf_set_noise_psd(vaenmf_plan* p, const float* Vb) {
  VN_REQUIRE(p != nullptr, "null plan");
  p->Vb_ext = Vb;
  return 0;
}

// ---- the graph cache of vaenmf_em_run (VnEmGraphs, common.h) ----
// The kernels' arguments are values and device pointers; a signature (buffers, shapes, counts) is captured at its second
// appearance and replayed from then on (a few signatures are kept).  Contents that change from batch to batch -- spectrogram,
// seeds, frame tables -- live behind those pointers and are read at run time.
namespace {
constexpr size_t MAX_GRAPHS = 4, MAX_SEEN = 8;

struct EmCall {                                         // the arguments of one vaenmf_em_run
  const float* X2; float *W, *Ht, *g, *Z; const float* B1; float* Zs;
  int32_t Rcap, niter, nsE, biE, nsWF, biWF; float var_rw;
  const float* X; float *S_hat, *N_hat; double* cost;
};

VnEmGraphs::Key em_graph_key(const vaenmf_plan* p, const EmCall& c, bool stored, const VnSwitches& sw) {
  auto u64 = [](const void* q) { return (uint64_t)(uintptr_t)q; };
  uint32_t vbits;
  memcpy(&vbits, &c.var_rw, 4);
  uint64_t fo_hash = 1469598103934665603ull;            // the batch's frame offsets (FNV-1a): launches derive grids and chunk tables from them
  for (int32_t v : p->h_frame_off) { fo_hash ^= (uint64_t)(uint32_t)v; fo_hash *= 1099511628211ull; }
  return {fo_hash,
      u64(c.X2), u64(c.W), u64(c.Ht), u64(c.g), u64(c.Z), u64(c.B1), u64(c.Zs), u64(c.X), u64(c.S_hat), u64(c.N_hat), u64(c.cost),
      (uint64_t)c.Rcap, (uint64_t)c.niter, (uint64_t)c.nsE, (uint64_t)c.biE, (uint64_t)c.nsWF, (uint64_t)c.biWF, (uint64_t)vbits, (uint64_t)stored,
      (uint64_t)p->NT, (uint64_t)p->n_utt, (uint64_t)p->n_wtiles, (uint64_t)p->n_tiles, u64(p->VsS), u64(p->src), u64(p->Vb_ext),
      (uint64_t)p->VsS_cap, (uint64_t)p->Rcap_store, u64(p->w1f), u64(p->w2f), u64(p->w3f), u64(p->w3c), u64(p->b3c), u64(p->b1),
      u64(p->d_wt_utt), u64(p->d_wt_n0), u64(p->d_wt_cnt), u64(p->d_frame_off), u64(p->d_frame_utt), u64(p->d_frame_loc), u64(p->d_tile_utt),
      u64(p->d_tile_n0), u64(p->d_tile_cnt), u64(p->d_utt_seed), u64(p->A1), u64(p->P), u64(p->normW), u64(p->wpart), u64(p->cost_frames), u64(p->w3n), u64(p->w1y), u64(p->b2), u64(p->b3),
      u64(p->wpart64), u64(p->wpart16), u64(p->d_t64_n0), u64(p->d_t64_cnt), u64(p->d_t64_first), u64(p->d_t64_g0), (uint64_t)p->n_t64,
      (uint64_t)p->cfg.precision, (uint64_t)p->cfg.K, (uint64_t)p->cfg.F,
      (uint64_t)sw.wchain4, (uint64_t)sw.team_chain, (uint64_t)sw.wfused, (uint64_t)sw.wgroup, (uint64_t)(uint32_t)sw.wfused_grid,
      (uint64_t)(uint32_t)sw.grid_cap,
      (uint64_t)sw.keep_zs, (uint64_t)sw.store_aligned};
}
}  // namespace

VnEmGraphs::Graph* VnEmGraphs::find(const Key& key) {
  for (auto& gph : cache)
    if (gph.key == key) return &gph;
  return nullptr;
}

bool VnEmGraphs::first_seen(const Key& key) {
  for (auto& k : seen) if (k == key) return false;
  if (seen.size() >= MAX_SEEN) seen.erase(seen.begin());
  seen.push_back(key);
  return true;
}

VnEmGraphs::Graph* VnEmGraphs::insert(const Key& key, hipGraphExec_t exec, int chain_kernel, int w_fused) {
  if (cache.size() >= MAX_GRAPHS) {                     // evict the least recently used
    size_t lru = 0;
    for (size_t i = 1; i < cache.size(); ++i) if (cache[i].used < cache[lru].used) lru = i;
    (void)hipGraphExecDestroy(cache[lru].exec);
    cache.erase(cache.begin() + lru);
  }
  cache.push_back({key, exec, 0, chain_kernel, w_fused});
  return &cache.back();
}

void VnEmGraphs::release() {
  for (auto& gph : cache) if (gph.exec) (void)hipGraphExecDestroy(gph.exec);
  cache.clear();
  if (cap_stream) (void)hipStreamDestroy(cap_stream);
  cap_stream = nullptr;
}

// the body of vaenmf_em_run: every launch on `stream`
static int em_run_body(vaenmf_plan* p, const EmCall& c, bool stored, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  vaenmf_rng rng = {VAENMF_RNG_DEVICE, 0, nullptr, nullptr};
  // the per-frame cost sums of VN_COST_CHUNK iterations are kept (one row of the plan's cost buffer each) and reduced to
  // cost[u][it] by ONE launch per chunk instead of one per iteration
  const size_t cstride = (size_t)p->cfg.max_frames;
  // With the sample-variance store on, the M-step never looks at the E-step's latent samples: the wave-private chain kernels
  // then do not record them (Zs = NULL: 123 MB of writes per launch at the bench shape that nothing reads); the Wiener chain
  // below records its own, which is what Zs holds after the reference's run() too (mcem.py:173, :477-482).
  float* Zs_e = (stored && !vn_switches().keep_zs &&
                 (p->wide || (vn_wchain_supported(p) &&
                              vaenmf_wchain_addressable(p->NT, c.Rcap, c.nsE + c.biE, p->Fs, p->Kp, p->n_utt, 0)))) ? nullptr : c.Zs;
  for (int it = 0; it < c.niter; ++it) {                // EM.run, mcem.py:159-165
    rng.call = (uint32_t)it;
    double* cf = p->cost_frames + (size_t)(it % VN_COST_CHUNK) * cstride;
    if (int e = vaenmf_mh_chain(p, c.X2, c.W, c.Ht, c.g, c.Z, 1, c.B1, Zs_e, c.Rcap, c.nsE, c.biE, c.var_rw, &rng, nullptr, stream)) return e;
    if (int e = stored ? vaenmf_m_step_stored(p, c.X2, c.W, c.Ht, c.g, cf, stream)
                       : vaenmf_m_step(p, c.X2, c.W, c.Ht, c.g, c.Zs, c.Rcap, c.nsE, c.B1, cf, stream)) return e;
    if (c.cost && ((it + 1) % VN_COST_CHUNK == 0 || it + 1 == c.niter)) {
      const int it0 = it - it % VN_COST_CHUNK;
      if (int e2 = vn_launch_cost_reduce(p, p->cost_frames, cstride, it - it0 + 1, c.nsE, c.cost, c.niter, it0, st)) return e2;
    }
  }
  rng.call = (uint32_t)c.niter;                         // compute_WF(sample=True), mcem.py:173
  if (int e = vaenmf_mh_chain(p, c.X2, c.W, c.Ht, c.g, c.Z, 0, c.B1, c.Zs, c.Rcap, c.nsWF, c.biWF, c.var_rw, &rng, nullptr, stream)) return e;
  if (stored) return vaenmf_wiener_stored(p, c.W, c.Ht, c.g, c.X, c.S_hat, c.N_hat, nullptr, nullptr, stream);
  return vaenmf_wiener(p, c.X2, c.W, c.Ht, c.g, c.Zs, c.Rcap, c.nsWF, c.B1, c.X, c.S_hat, c.N_hat, nullptr, nullptr, stream);
}

// replay of a captured call, and the host-side state an eager call leaves behind
static int em_graph_launch(vaenmf_plan* p, VnEmGraphs::Graph& gph, const EmCall& c, bool stored, hipStream_t st) {
  VN_CHECK_HIP(hipGraphLaunch(gph.exec, st));
  gph.used = ++p->graphs.tick;
  if (stored) { p->store_R = c.nsWF; p->store_Rs = c.nsWF + 1; p->store_lay = vn_store_layout(p, c.nsWF + 1, c.B1 != nullptr); }
  p->last_chain_kernel = gph.chain_kernel;
  p->last_w_fused = gph.w_fused;
  p->graphs.last = 1;
  return 0;
}

// em_run_body captured on the plan's own stream (the caller's may be the null stream) and instantiated; null, and no more
// graphs on this plan, when any step fails
static hipGraphExec_t em_graph_capture(vaenmf_plan* p, const EmCall& c, bool stored) {
  VnEmGraphs& G = p->graphs;
  auto fail = [&]() { (void)hipGetLastError(); G.off = true; return (hipGraphExec_t) nullptr; };
  if (!G.cap_stream && hipStreamCreateWithFlags(&G.cap_stream, hipStreamNonBlocking) != hipSuccess) return fail();
  if (hipStreamBeginCapture(G.cap_stream, hipStreamCaptureModeThreadLocal) != hipSuccess) return fail();
  hipGraph_t graph = nullptr;
  const int rc = em_run_body(p, c, stored, (void*)G.cap_stream);
  const hipError_t ec = hipStreamEndCapture(G.cap_stream, &graph);
  hipGraphExec_t exec = nullptr;
  const bool ok = rc == 0 && ec == hipSuccess && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess && exec;
  if (graph) (void)hipGraphDestroy(graph);
  return ok ? exec : fail();
}

extern "C" int vaenmf_em_run(vaenmf_plan* p, const float* X2, float* W, float* Ht, float* g, float* Z, const float* B1,
                             float* Zs, int32_t Rcap, int32_t niter, int32_t nsE, int32_t biE, int32_t nsWF, int32_t biWF,
                             float var_rw, const float* X, float* S_hat, float* N_hat, double* cost, void* stream) {
  if (int e = check_bound(p)) return e;
  VN_REQUIRE(nsE <= Rcap && nsWF <= Rcap, "Rcap=%d too small for nsE=%d / nsWF=%d", Rcap, nsE, nsWF);
  const EmCall c = {X2, W, Ht, g, Z, B1, Zs, Rcap, niter, nsE, biE, nsWF, biWF, var_rw, X, S_hat, N_hat, cost};
  // with the sample store on (vaenmf_sample_store), the chain leaves the samples' variances in HBM and the
  // M-step / Wiener filter stream them; otherwise they decode Zs again
  // (a batch too large for the store's 32-bit element offsets decodes; every F the plan accepts, <= 640, is in the streaming
  // kernels' bin range)
  const int esz = p->cfg.precision == VAENMF_PREC_BF16X3 ? 4 : 2;
  auto fits = [&](int ns) { return vn_store_bytes(vn_store_layout(p, ns + 1, B1 != nullptr), (size_t)p->NT + 1, esz) < 0xE0000000ull; };
  const bool want = p->store_on, stored = want && fits(nsE) && fits(nsWF);
  // a wide plan has no decoding M-step / Wiener kernels to fall back to
  VN_REQUIRE(!p->wide || want, "vaenmf_em_run on a wide decoder plan streams the sample store: switch it on with vaenmf_sample_store first");
  VN_REQUIRE(!p->wide || stored, "vaenmf_em_run on a wide decoder plan: the sample store of %d frames passes the 32-bit offsets of the "
             "streaming kernels and there is no decoding path for wide decoders; bind a smaller batch", p->NT);
  p->store_on = stored;
  p->last_m_step_path = stored ? 1 : 2;               // VAENMF_Q_MSTEP_PATH: the caller can see a fall back to decoding
  struct Restore { vaenmf_plan* p; bool v; ~Restore() { p->store_on = v; } } restore{p, want};
  auto eager = [&]() { return em_run_body(p, c, stored, stream); };

  static const bool graphs_on = []() { const char* e = getenv("VAENMF_GRAPH"); return !(e && e[0] == '0'); }();
  VnEmGraphs& G = p->graphs;
  G.last = 0;
  if (!graphs_on || G.off || p->prof_on) return eager();
  const VnEmGraphs::Key key = em_graph_key(p, c, stored, vn_switches());    // the switches: kernel choices the captured launches depend on
  if (VnEmGraphs::Graph* gph = G.find(key)) return em_graph_launch(p, *gph, c, stored, (hipStream_t)stream);
  if (G.first_seen(key)) return eager();                // first call of this signature: eager (it also sets every kernel attribute)
  const hipGraphExec_t exec = em_graph_capture(p, c, stored);             // second appearance of the signature: capture
  if (!exec) return eager();
  return em_graph_launch(p, *G.insert(key, exec, p->last_chain_kernel, p->last_w_fused), c, stored, (hipStream_t)stream);
}
