// STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016) for ragged batches of 10 kHz signals -- stands where the reference
// calls pystoi (scripts/run_metrics_M2.py:117: stoi(s_t, s_hat_t, fs, extended=True)).  The definition is in
// include/vaenmf.h; this file is its dataflow.  Everything that feeds a decision or a sum is float64.
//
//   stoi_energy_kernel   one wavefront per frame of the clean signal: ||w x|| (fixed butterfly over the 64 lanes)
//   stoi_scan_kernel     one workgroup per utterance: the loudest frame, then the frames in chunks of 256 with a carried
//                        prefix: keep[], src[] (the kept frames in order), counts = {n_frames, k, J}
//   stoi_tob_kernel      one workgroup per rebuilt frame and signal: the two-term gather of the overlap-add, the window, a
//                        512-point FFT in LDS (fft_lds), 15 band sums over consecutive bins, one row of 16 doubles
//   stoi_segment_kernel  one workgroup per 16 consecutive segments of an utterance: their 45 frames of both signals staged
//                        in LDS, one wavefront per segment: row / column normalisation (ESTOI) or the clipped row
//                        correlation (STOI), the 30 (15) partial sums added by one lane in ascending order
//   stoi_sum_kernel      one workgroup per utterance: its segments' sums in a fixed tree, d
//
// No atomics; every output has its own lanes and its own order of additions, so an utterance's bits do not depend on its
// batch.  k, M and J never leave the device: the grids cover the worst case k = n_frames and a workgroup without work
// exits on the count it reads.  Which utterance a workgroup serves it finds by bisection in offset tables that the host
// derives from the sample offsets and hands to the device as kernel arguments (no host buffer outlives the call, nothing
// is allocated).  The window and the FFT twiddles are a 6 KiB table per device, built on the host in long double at the
// first call.
#include <math.h>
#include <map>
#include <mutex>
#include <vector>
#include "common.h"

namespace {

constexpr int ST_FRAME = 256, ST_HOP = 128, ST_NFFT = 512, ST_BITS = 9, ST_BANDS = 15, ST_ROW = 16, ST_SEG = 30;
constexpr int ST_FS = 10000, ST_MIN_FREQ = 150;
constexpr double ST_EPS = 2.220446049250313e-16;       // 2^-52
constexpr double ST_DYN_RANGE = 40.0;
constexpr double ST_CLIP = 6.623413251903491;          // 1 + 10^(15/20)
constexpr double ST_NO_SCORE = 1e-5;
constexpr int ST_WG_SEGS = 16, ST_WAVES = 4;           // segments per workgroup of stoi_segment_kernel, its wavefronts
constexpr int ST_STAGE = ST_WG_SEGS + ST_SEG - 1;      // frames those segments cover
constexpr int ST_PAD = ST_ROW + 1;                     // row stride of the per-wave scratch (lanes walk it by rows)

// offset tables, int64 [ST_TABS][n_utt + 1]: samples, frames, rows of tob (max_spec_frames), segments (max_segments),
// workgroups of stoi_segment_kernel
enum { TAB_SAMP = 0, TAB_FRAME = 1, TAB_SPEC = 2, TAB_SEG = 3, TAB_BLK = 4, ST_TABS = 5 };
constexpr int ST_CHUNK = 384;                          // table entries one stoi_put_kernel launch carries (3 KiB of arguments)
struct TabChunk { int64_t v[ST_CHUNK]; };
struct Bands { int32_t lo[ST_ROW], hi[ST_ROW]; };
struct StoiTables { const double *w, *twr, *twi; };   // [256] window, [256] cos / sin(-2 pi t / 512)

__global__ void stoi_put_kernel(TabChunk c, int n, int64_t* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = c.v[i];
}

// the utterance u with off[u] <= i < off[u+1], for 0 <= i < off[n_utt]
__device__ __forceinline__ int find_utt(const int64_t* __restrict__ off, int n_utt, int64_t i) {
  int lo = 0, hi = n_utt;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void stoi_energy_kernel(const float* __restrict__ x, const int64_t* __restrict__ tab, int n_utt,
                                                          int64_t n_frames_total, StoiTables T, double* __restrict__ norms) {
  const int lane = threadIdx.x & 63;
  const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= n_frames_total) return;                       // the whole wavefront
  const int64_t* foff = tab + (size_t)TAB_FRAME * (n_utt + 1);
  const int u = find_utt(foff, n_utt, f);
  const float* s = x + tab[u] + (f - foff[u]) * ST_HOP;  // 128 j + 255 < T - 1 for every frame j < n_frames
  double acc = 0.0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const double v = T.w[lane + 64 * t] * (double)s[lane + 64 * t];
    acc += v * v;
  }
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
  if (lane == 0) norms[f] = sqrt(acc);
}

__device__ __forceinline__ double level_db(double norm) { return 20.0 * log10(norm + ST_EPS); }

__global__ __launch_bounds__(256) void stoi_scan_kernel(const double* __restrict__ norms, const int64_t* __restrict__ tab, int n_utt,
                                                        int32_t* __restrict__ keep, int32_t* __restrict__ src,
                                                        int32_t* __restrict__ counts) {
  __shared__ double wmax[4];
  __shared__ int wsum[4];
  const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t* foff = tab + (size_t)TAB_FRAME * (n_utt + 1);
  const int64_t f0 = foff[u];
  const int nf = (int)(foff[u + 1] - f0);
  double mx = -INFINITY;
  for (int j = tid; j < nf; j += 256) mx = fmax(mx, level_db(norms[f0 + j]));
  for (int m = 32; m >= 1; m >>= 1) mx = fmax(mx, __shfl_xor(mx, m));
  if (lane == 0) wmax[wave] = mx;
  __syncthreads();
  mx = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
  int carry = 0;                                         // frames kept before this chunk
  for (int base = 0; base < nf; base += 256) {
    const int j = base + tid;
    const bool kp = j < nf && mx - ST_DYN_RANGE - level_db(norms[f0 + j]) < 0.0;
    const unsigned long long b = __ballot(kp);
    if (lane == 0) wsum[wave] = __popcll(b);
    __syncthreads();
    int before = __popcll(b & ((1ull << lane) - 1ull)), total = 0;
    for (int i = 0; i < 4; ++i) {
      if (i < wave) before += wsum[i];
      total += wsum[i];
    }
    if (j < nf) {
      keep[f0 + j] = kp ? 1 : 0;
      if (kp) src[f0 + carry + before] = j;              // carry + before < k <= nf
    }
    carry += total;
    __syncthreads();
  }
  if (tid == 0) {
    counts[3 * u] = nf;
    counts[3 * u + 1] = carry;
    counts[3 * u + 2] = carry - 1 >= ST_SEG ? carry - ST_SEG : 0;      // J = M - 29, M = k - 1
  }
}

__global__ __launch_bounds__(256) void stoi_tob_kernel(const float* __restrict__ clean, const float* __restrict__ proc,
                                                       const int64_t* __restrict__ tab, int n_utt, const int32_t* __restrict__ src,
                                                       const int32_t* __restrict__ counts, StoiTables T, Bands bands,
                                                       double* __restrict__ tob_x, double* __restrict__ tob_y) {
  __shared__ double re[ST_NFFT], im[ST_NFFT], twr[ST_NFFT / 2], twi[ST_NFFT / 2];
  const int64_t* foff = tab + (size_t)TAB_FRAME * (n_utt + 1);
  const int64_t* poff = tab + (size_t)TAB_SPEC * (n_utt + 1);
  const int64_t row = blockIdx.x;
  const int u = find_utt(poff, n_utt, row);
  const int m = (int)(row - poff[u]);
  if (m >= counts[3 * u + 1] - 1) return;                // the whole workgroup: rows >= M stay as they are
  const float* s = (blockIdx.y ? proc : clean) + tab[u];
  const int32_t* sr = src + foff[u];
  const int t = threadIdx.x;
  twr[t] = T.twr[t];
  twi[t] = T.twi[t];
  // sample 128 q + r of the rebuilt signal: frame q of the kept ones (q <= m + 1 <= k - 1) and, from q = 1 on, frame q - 1
  const int r = t & (ST_HOP - 1), q = m + (t >> 7);
  double v = 0.0;
  if (q >= 1) v = T.w[r + ST_HOP] * (double)s[(int64_t)ST_HOP * sr[q - 1] + r + ST_HOP];
  v += T.w[r] * (double)s[(int64_t)ST_HOP * sr[q] + r];
  re[bitrev(t, ST_BITS)] = v * T.w[t];
  im[bitrev(t, ST_BITS)] = 0.0;
  re[bitrev(t + ST_FRAME, ST_BITS)] = 0.0;
  im[bitrev(t + ST_FRAME, ST_BITS)] = 0.0;
  __syncthreads();
  fft_lds(re, im, twr, twi, ST_NFFT, ST_BITS, 1);
  if (t < ST_ROW) {
    double acc = 0.0;
    if (t < ST_BANDS)
      for (int bin = bands.lo[t]; bin < bands.hi[t]; ++bin) acc += re[bin] * re[bin] + im[bin] * im[bin];
    (blockIdx.y ? tob_y : tob_x)[row * ST_ROW + t] = sqrt(acc);
  }
}

__global__ __launch_bounds__(256) void stoi_segment_kernel(const double* __restrict__ tob_x, const double* __restrict__ tob_y,
                                                           const int64_t* __restrict__ tab, int n_utt,
                                                           const int32_t* __restrict__ counts, int extended,
                                                           double* __restrict__ seg_d) {
  __shared__ double sx[ST_STAGE * ST_ROW], sy[ST_STAGE * ST_ROW];
  __shared__ double nx[ST_WAVES][ST_SEG * ST_PAD], ny[ST_WAVES][ST_SEG * ST_PAD];
  __shared__ double part[ST_WAVES][32];
  const int64_t* poff = tab + (size_t)TAB_SPEC * (n_utt + 1);
  const int64_t* goff = tab + (size_t)TAB_SEG * (n_utt + 1);
  const int64_t* boff = tab + (size_t)TAB_BLK * (n_utt + 1);
  const int u = find_utt(boff, n_utt, blockIdx.x);
  const int s0 = (int)(blockIdx.x - boff[u]) * ST_WG_SEGS;
  int J = counts[3 * u + 2];
  if (J > goff[u + 1] - goff[u]) J = (int)(goff[u + 1] - goff[u]);    // never past the utterance's rows, whatever counts holds
  if (s0 >= J) return;                                   // the whole workgroup
  const int ns = J - s0 < ST_WG_SEGS ? J - s0 : ST_WG_SEGS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row0 = (size_t)(poff[u] + s0) * ST_ROW;   // rows s0 .. s0 + ns + 28 <= J + 28 = M - 1
  for (int i = tid; i < (ns + ST_SEG - 1) * ST_ROW; i += 256) {
    sx[i] = tob_x[row0 + i];
    sy[i] = tob_y[row0 + i];
  }
  __syncthreads();
  for (int it = 0; it < ST_WG_SEGS / ST_WAVES; ++it) {
    const int sg = it * ST_WAVES + wave;
    const bool on = sg < ns;
    const double* x = sx + sg * ST_ROW;                  // frame f, band b of the segment: x[f * ST_ROW + b]
    const double* y = sy + sg * ST_ROW;
    int n_part;
    if (extended) {
      // rows: lanes 0 .. 14 the bands of the clean signal, lanes 16 .. 30 those of the processed one
      if (on && lane < 32 && (lane & 15) < ST_BANDS) {
        const double* v = (lane >> 4) ? y : x;
        double* o = (lane >> 4) ? ny[wave] : nx[wave];
        const int b = lane & 15;
        double mean = 0.0, n2 = 0.0;
        for (int f = 0; f < ST_SEG; ++f) mean += v[f * ST_ROW + b];
        mean /= ST_SEG;
        for (int f = 0; f < ST_SEG; ++f) {
          const double c = v[f * ST_ROW + b] - mean;
          n2 += c * c;
        }
        const double nrm = sqrt(n2);
        for (int f = 0; f < ST_SEG; ++f) o[f * ST_PAD + b] = nrm > 0.0 ? (v[f * ST_ROW + b] - mean) / nrm : 0.0;
      }
      __syncthreads();
      // columns: lane f the frame f of both signals
      if (on && lane < ST_SEG) {
        const double* a = nx[wave] + lane * ST_PAD;
        const double* c = ny[wave] + lane * ST_PAD;
        double ma = 0.0, mc = 0.0, na = 0.0, nc = 0.0, dot = 0.0;
        for (int b = 0; b < ST_BANDS; ++b) { ma += a[b]; mc += c[b]; }
        ma /= ST_BANDS; mc /= ST_BANDS;
        for (int b = 0; b < ST_BANDS; ++b) {
          const double da = a[b] - ma, dc = c[b] - mc;
          na += da * da; nc += dc * dc; dot += da * dc;
        }
        const double nrm = sqrt(na) * sqrt(nc);
        part[wave][lane] = nrm > 0.0 ? dot / nrm : 0.0;
      }
      n_part = ST_SEG;
    } else {
      // lane b the band b of both signals
      if (on && lane < ST_BANDS) {
        double ex = 0.0, ey = 0.0;
        for (int f = 0; f < ST_SEG; ++f) {
          const double a = x[f * ST_ROW + lane], c = y[f * ST_ROW + lane];
          ex += a * a; ey += c * c;
        }
        const double g = sqrt(ex) / (sqrt(ey) + ST_EPS);
        double ma = 0.0, mc = 0.0;
        for (int f = 0; f < ST_SEG; ++f) {
          const double a = x[f * ST_ROW + lane];
          ma += a;
          mc += fmin(g * y[f * ST_ROW + lane], a * ST_CLIP);
        }
        ma /= ST_SEG; mc /= ST_SEG;
        double na = 0.0, nc = 0.0, dot = 0.0;
        for (int f = 0; f < ST_SEG; ++f) {
          const double a = x[f * ST_ROW + lane];
          const double da = a - ma, dc = fmin(g * y[f * ST_ROW + lane], a * ST_CLIP) - mc;
          na += da * da; nc += dc * dc; dot += da * dc;
        }
        part[wave][lane] = dot / ((sqrt(na) + ST_EPS) * (sqrt(nc) + ST_EPS));
      }
      n_part = ST_BANDS;
    }
    __syncthreads();
    if (on && lane == 0) {
      double total = 0.0;
      for (int i = 0; i < n_part; ++i) total += part[wave][i];
      seg_d[goff[u] + s0 + sg] = total;                  // s0 + sg < J <= max_segments
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void stoi_sum_kernel(const double* __restrict__ seg_d, const int64_t* __restrict__ tab, int n_utt,
                                                       const int32_t* __restrict__ counts, int extended, double* __restrict__ d) {
  __shared__ double red[256];
  const int u = blockIdx.x, tid = threadIdx.x;
  const int64_t* goff = tab + (size_t)TAB_SEG * (n_utt + 1);
  int J = counts[3 * u + 2];
  if (J > goff[u + 1] - goff[u]) J = (int)(goff[u + 1] - goff[u]);
  if (J <= 0) {                                          // fewer than 30 frames: pystoi's warning value
    if (tid == 0) d[u] = ST_NO_SCORE;
    return;
  }
  double acc = 0.0;
  for (int i = tid; i < J; i += 256) acc += seg_d[goff[u] + i];
  red[tid] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) d[u] = red[0] / ((extended ? (double)ST_SEG : (double)ST_BANDS) * J);
}

// ---------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------
void geometry(int64_t T, int64_t* nf, int64_t* spec, int64_t* seg) {
  *nf = T > ST_FRAME ? (T - ST_FRAME + ST_HOP - 1) / ST_HOP : 0;      // starts 0, 128, .. < T - 256
  *spec = *nf > 0 ? *nf - 1 : 0;
  *seg = *spec >= ST_SEG ? *spec - (ST_SEG - 1) : 0;
}

void band_bins(int32_t* lo, int32_t* hi) {
  for (int b = 0; b < ST_BANDS; ++b)
    for (int e = 0; e < 2; ++e) {
      const double edge = (double)ST_MIN_FREQ * pow(2.0, (2.0 * b + (e ? 1.0 : -1.0)) / 6.0);
      int best = 0;
      double dbest = INFINITY;
      for (int i = 0; i <= ST_NFFT / 2; ++i) {
        const double f = (double)ST_FS * i / ST_NFFT, dd = (f - edge) * (f - edge);
        if (dd < dbest) { dbest = dd; best = i; }        // the first index on a tie
      }
      (e ? hi : lo)[b] = best;
    }
}

// Bytes into the work buffer; doubles and the tables first, so that an 8-byte aligned buffer aligns them all
struct Layout {
  int64_t NF, NS, NG, NB;                                // frames, rows of tob, segments, workgroups of the segment kernel
  size_t tab, norms, seg_d, tob_x, tob_y, src, keep, counts, total;
};

int make_layout(int32_t n_utt, const int64_t* off, const char* who, Layout* L, std::vector<int64_t>* tabs) {
  VN_REQUIRE(n_utt >= 0, "%s: n_utt=%d", who, n_utt);
  VN_REQUIRE(n_utt == 0 || off, "%s: null sample_offsets", who);
  const size_t no = (size_t)n_utt + 1;
  std::vector<int64_t> t(ST_TABS * no, 0);
  for (int32_t u = 0; u < n_utt; ++u) {
    const int64_t T = off[u + 1] - off[u];
    VN_REQUIRE(T >= 0, "%s: sample_offsets decrease at utterance %d", who, u);
    int64_t nf, spec, seg;
    geometry(T, &nf, &spec, &seg);
    t[TAB_SAMP * no + u] = off[u];
    t[TAB_SAMP * no + u + 1] = off[u + 1];
    t[TAB_FRAME * no + u + 1] = t[TAB_FRAME * no + u] + nf;
    t[TAB_SPEC * no + u + 1] = t[TAB_SPEC * no + u] + spec;
    t[TAB_SEG * no + u + 1] = t[TAB_SEG * no + u] + seg;
    t[TAB_BLK * no + u + 1] = t[TAB_BLK * no + u] + (seg + ST_WG_SEGS - 1) / ST_WG_SEGS;
  }
  L->NF = t[TAB_FRAME * no + n_utt]; L->NS = t[TAB_SPEC * no + n_utt];
  L->NG = t[TAB_SEG * no + n_utt]; L->NB = t[TAB_BLK * no + n_utt];
  VN_REQUIRE(L->NF <= 0x7fffffff, "%s: %lld frames exceed the grid limit", who, (long long)L->NF);
  size_t p = 0;
  L->tab = p; p += 8 * t.size();
  L->norms = p; p += 8 * (size_t)L->NF;
  L->seg_d = p; p += 8 * (size_t)L->NG;
  L->tob_x = p; p += 8 * (size_t)L->NS * ST_ROW;
  L->tob_y = p; p += 8 * (size_t)L->NS * ST_ROW;
  L->src = p; p += 4 * (size_t)L->NF;
  L->keep = p; p += 4 * (size_t)L->NF;
  L->counts = p; p += 12 * (size_t)n_utt;
  L->total = p;
  if (tabs) tabs->swap(t);
  return 0;
}

int check_work(const Layout& L, const void* work, int64_t work_bytes, const char* who) {
  VN_REQUIRE(work && ((uintptr_t)work & 7) == 0, "%s: work must be a device buffer aligned to 8 bytes", who);
  VN_REQUIRE(work_bytes >= (int64_t)L.total, "%s: work_bytes=%lld, vaenmf_stoi_work_bytes gives %lld", who, (long long)work_bytes,
             (long long)L.total);
  return 0;
}

int put_tables(const std::vector<int64_t>& tabs, int64_t* d_tab, hipStream_t st) {
  for (size_t i = 0; i < tabs.size(); i += ST_CHUNK) {
    TabChunk c;
    const int n = (int)(tabs.size() - i < (size_t)ST_CHUNK ? tabs.size() - i : ST_CHUNK);
    for (int j = 0; j < ST_CHUNK; ++j) c.v[j] = j < n ? tabs[i + j] : 0;
    hipLaunchKernelGGL(stoi_put_kernel, dim3((ST_CHUNK + 127) / 128), dim3(128), 0, st, c, n, d_tab + i);
    VN_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

// The window and twiddle table of the current device, built at the first call (one upload) and kept for the life of the process
int get_tables(StoiTables* out) {
  static std::mutex mu;
  static std::map<int, StoiTables> tables;
  int dev = 0;
  VN_CHECK_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  auto it = tables.find(dev);
  if (it == tables.end()) {
    const long double pi = 3.14159265358979323846264338327950288L;
    std::vector<double> h(3 * ST_FRAME);
    for (int i = 0; i < ST_FRAME; ++i) {
      h[i] = (double)(0.5L - 0.5L * cosl(2.0L * pi * (long double)(i + 1) / (ST_FRAME + 1)));   // symmetric Hann of 258 points, ends dropped
      h[ST_FRAME + i] = (double)cosl(-2.0L * pi * (long double)i / ST_NFFT);
      h[2 * ST_FRAME + i] = (double)sinl(-2.0L * pi * (long double)i / ST_NFFT);
    }
    double* d = nullptr;
    VN_CHECK_HIP(hipMalloc(&d, h.size() * sizeof(double)));
    const hipError_t ec = hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
    if (ec != hipSuccess) {
      (void)hipFree(d);
      VN_CHECK_HIP(ec);
    }
    it = tables.emplace(dev, StoiTables{d, d + ST_FRAME, d + 2 * ST_FRAME}).first;
  }
  *out = it->second;
  return 0;
}

// stages 1-3 with the tables already at d_tab
int launch_tob(const float* clean, const float* proc, int32_t n_utt, const Layout& L, const int64_t* d_tab, double* norms,
               int32_t* src, int32_t* keep, int32_t* counts, double* tob_x, double* tob_y, hipStream_t st) {
  StoiTables T;
  if (int rc = get_tables(&T)) return rc;
  if (L.NF > 0) {
    hipLaunchKernelGGL(stoi_energy_kernel, dim3((unsigned)((L.NF + 3) / 4)), dim3(256), 0, st, clean, d_tab, n_utt, L.NF, T, norms);
    VN_CHECK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(stoi_scan_kernel, dim3((unsigned)n_utt), dim3(256), 0, st, norms, d_tab, n_utt, keep, src, counts);
  VN_CHECK_HIP(hipGetLastError());
  if (L.NS > 0) {
    Bands bands{};
    band_bins(bands.lo, bands.hi);
    hipLaunchKernelGGL(stoi_tob_kernel, dim3((unsigned)L.NS, 2), dim3(256), 0, st, clean, proc, d_tab, n_utt, src, counts, T, bands,
                       tob_x, tob_y);
    VN_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

// stages 4-5 with the tables already at d_tab
int launch_segments(const double* tob_x, const double* tob_y, const int32_t* counts, int32_t n_utt, const Layout& L,
                    const int64_t* d_tab, int32_t extended, double* seg_d, double* d, hipStream_t st) {
  if (L.NB > 0) {
    hipLaunchKernelGGL(stoi_segment_kernel, dim3((unsigned)L.NB), dim3(256), 0, st, tob_x, tob_y, d_tab, n_utt, counts, extended, seg_d);
    VN_CHECK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(stoi_sum_kernel, dim3((unsigned)n_utt), dim3(256), 0, st, seg_d, d_tab, n_utt, counts, extended, d);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

template <class T>
T* at(void* work, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(work) + off); }

}  // namespace

extern "C" int vaenmf_stoi_geometry(int64_t n_samples, int32_t* n_frames, int32_t* max_spec_frames, int32_t* max_segments) {
  VN_REQUIRE(n_frames && max_spec_frames && max_segments, "vaenmf_stoi_geometry: bad arguments");
  VN_REQUIRE(n_samples >= 0, "vaenmf_stoi_geometry: n_samples=%lld", (long long)n_samples);
  int64_t nf, spec, seg;
  geometry(n_samples, &nf, &spec, &seg);
  VN_REQUIRE(nf <= 0x7fffffff, "vaenmf_stoi_geometry: %lld samples are %lld frames, more than 2^31 - 1", (long long)n_samples, (long long)nf);
  *n_frames = (int32_t)nf; *max_spec_frames = (int32_t)spec; *max_segments = (int32_t)seg;
  return 0;
}

extern "C" int vaenmf_stoi_bands(int32_t* lo, int32_t* hi) {
  VN_REQUIRE(lo && hi, "vaenmf_stoi_bands: bad arguments");
  band_bins(lo, hi);
  return 0;
}

extern "C" int64_t vaenmf_stoi_work_bytes(int32_t n_utt, const int64_t* sample_offsets) {
  Layout L;
  if (make_layout(n_utt, sample_offsets, "vaenmf_stoi_work_bytes", &L, nullptr)) return -1;
  return (int64_t)L.total;
}

extern "C" int vaenmf_stoi_tob(const float* clean, const float* proc, int32_t n_utt, const int64_t* sample_offsets, int32_t* keep,
                               int32_t* counts, double* tob_x, double* tob_y, void* work, int64_t work_bytes, void* stream) {
  Layout L;
  std::vector<int64_t> tabs;
  if (int rc = make_layout(n_utt, sample_offsets, "vaenmf_stoi_tob", &L, &tabs)) return rc;
  if (n_utt == 0) return 0;
  if (int rc = check_work(L, work, work_bytes, "vaenmf_stoi_tob")) return rc;
  VN_REQUIRE(counts && (L.NF == 0 || (clean && proc && keep)) && (L.NS == 0 || (tob_x && tob_y)), "vaenmf_stoi_tob: null buffers");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = put_tables(tabs, at<int64_t>(work, L.tab), st)) return rc;
  return launch_tob(clean, proc, n_utt, L, at<int64_t>(work, L.tab), at<double>(work, L.norms), at<int32_t>(work, L.src), keep, counts,
                    tob_x, tob_y, st);
}

extern "C" int vaenmf_stoi_segments(const double* tob_x, const double* tob_y, const int32_t* counts, int32_t n_utt,
                                    const int64_t* sample_offsets, int32_t extended, double* d, void* work, int64_t work_bytes,
                                    void* stream) {
  Layout L;
  std::vector<int64_t> tabs;
  if (int rc = make_layout(n_utt, sample_offsets, "vaenmf_stoi_segments", &L, &tabs)) return rc;
  if (n_utt == 0) return 0;
  if (int rc = check_work(L, work, work_bytes, "vaenmf_stoi_segments")) return rc;
  VN_REQUIRE(counts && d && (L.NG == 0 || (tob_x && tob_y)), "vaenmf_stoi_segments: null buffers");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = put_tables(tabs, at<int64_t>(work, L.tab), st)) return rc;
  return launch_segments(tob_x, tob_y, counts, n_utt, L, at<int64_t>(work, L.tab), extended != 0, at<double>(work, L.seg_d), d, st);
}

extern "C" int vaenmf_stoi_batch(const float* clean, const float* proc, int32_t n_utt, const int64_t* sample_offsets, int32_t extended,
                                 double* d, int32_t* counts, void* work, int64_t work_bytes, void* stream) {
  Layout L;
  std::vector<int64_t> tabs;
  if (int rc = make_layout(n_utt, sample_offsets, "vaenmf_stoi_batch", &L, &tabs)) return rc;
  if (n_utt == 0) return 0;
  if (int rc = check_work(L, work, work_bytes, "vaenmf_stoi_batch")) return rc;
  VN_REQUIRE(d && (L.NF == 0 || (clean && proc)), "vaenmf_stoi_batch: null buffers");
  hipStream_t st = (hipStream_t)stream;
  int64_t* d_tab = at<int64_t>(work, L.tab);
  int32_t* cnt = counts ? counts : at<int32_t>(work, L.counts);
  double *tx = at<double>(work, L.tob_x), *ty = at<double>(work, L.tob_y);
  if (int rc = put_tables(tabs, d_tab, st)) return rc;
  if (int rc = launch_tob(clean, proc, n_utt, L, d_tab, at<double>(work, L.norms), at<int32_t>(work, L.src), at<int32_t>(work, L.keep),
                          cnt, tx, ty, st))
    return rc;
  return launch_segments(tx, ty, cnt, n_utt, L, d_tab, extended != 0, at<double>(work, L.seg_d), d, st);
}
