// Batched rational-ratio resampler: scipy.signal.resample_poly(x, up, down, window=('kaiser', beta)) with zero padding
// (the reference resamples its noise with librosa.resample, python/dataset/qut_database.py / demand_database.py), in
// closed form.  With M = max(up, down), half = zeros M and the 2 half + 1 taps
//   h[i] = up s[i] w[i] / sum_j s[j] w[j],  t = i - half,  s = sin(pi t / M) / (pi t),  w = I0(beta sqrt(1 - (t/half)^2)) / I0(beta)
// output sample m of an utterance of n_in samples is
//   y[m] = sum_n x[n] h[half + m down - n up],  n in [0, n_in) with the tap index in [0, 2 half],  n_out = ceil(n_in up / down)
// summed in fp64 in ascending n and rounded once to float32: an utterance's bits do not depend on its batch.
//
// Tables: the taps are built once per (device, up, down, zeros, beta) on the host in long double, rounded to double and
// uploaded polyphase-major: row p = (half + m down) mod up holds h[p + j up], j = J-1 .. 0 (J = ceil((2 half + 1) / up)
// entries, indices past 2 half are zero and never read), so that a thread that walks n upwards walks its row upwards.
// One thread per output sample, 256 outputs of one utterance per workgroup; the workgroup stages the input span of its
// outputs in LDS, RS_CHUNK samples at a time.  Which utterance a workgroup serves comes from a block table built on the
// host from the offsets and kept on the device per batch shape.
#include <math.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>
#include <utility>
#include <vector>
#include "common.h"

namespace {

constexpr int RS_BLOCK = 256;        // outputs (threads) per workgroup
constexpr int RS_CHUNK = 4096;       // input samples staged in LDS at a time (16 KiB)
constexpr int RS_MAX_RATIO = 1024;   // largest up / down after reduction: a table of 20 * 1024 + 1 doubles
constexpr int RS_MAX_ZEROS = 64;
constexpr int RS_NOT_SUPPORTED = -3; // return code of a ratio over the limit

struct ResampleArgs {
  int up, down;
  int half;                 // zeros * max(up, down)
  int J;                    // entries per phase row
  const double* tab;        // [up][J]
};

__global__ __launch_bounds__(RS_BLOCK) void resample_kernel(const float* __restrict__ x, const int64_t* __restrict__ in_off,
                                                            const int64_t* __restrict__ out_off, const int32_t* __restrict__ blk_utt,
                                                            const int64_t* __restrict__ blk_m0, ResampleArgs a,
                                                            float* __restrict__ y) {
  __shared__ float xs[RS_CHUNK];
  const int u = blk_utt[blockIdx.x];
  const int64_t m0 = blk_m0[blockIdx.x];
  const int64_t ioff = in_off[u], n_in = in_off[u + 1] - ioff;
  const int64_t ooff = out_off[u], n_out = out_off[u + 1] - ooff;
  // inputs of output m: n = q - j for the taps p + j up <= 2 half, q = (half + m down) / up, p the remainder
  const int64_t m = m0 + threadIdx.x;
  const bool active = m < n_out;
  const int64_t c = a.half + m * a.down, q = c / a.up;
  const int p = (int)(c - q * a.up);
  int64_t n_lo = q - (2 * a.half - p) / a.up, n_hi = q;
  if (n_lo < 0) n_lo = 0;
  if (n_hi > n_in - 1) n_hi = n_in - 1;
  // span of the workgroup (both ends grow with m): first input of its first output .. last input of its last output
  const int64_t m1 = (m0 + RS_BLOCK < n_out ? m0 + RS_BLOCK : n_out) - 1;
  const int64_t c0 = a.half + m0 * a.down, q0 = c0 / a.up;
  int64_t b_lo = q0 - (2 * a.half - (c0 - q0 * a.up)) / a.up, b_hi = (a.half + m1 * a.down) / a.up;
  if (b_lo < 0) b_lo = 0;
  if (b_hi > n_in - 1) b_hi = n_in - 1;
  const double* __restrict__ row = a.tab + (size_t)p * a.J;
  const int64_t r0 = q - (a.J - 1);                      // input that meets row[0]
  double acc = 0.0;
  for (int64_t base = b_lo; base <= b_hi; base += RS_CHUNK) {
    const int64_t cnt = b_hi - base + 1 < RS_CHUNK ? b_hi - base + 1 : RS_CHUNK;
    __syncthreads();
    for (int i = threadIdx.x; i < cnt; i += RS_BLOCK) xs[i] = x[ioff + base + i];   // 0 <= base + i <= b_hi < n_in
    __syncthreads();
    if (active) {
      const int64_t lo = n_lo > base ? n_lo : base;
      const int64_t hi = n_hi < base + cnt - 1 ? n_hi : base + cnt - 1;
      for (int64_t n = lo; n <= hi; ++n) acc += (double)xs[n - base] * row[n - r0];
    }
  }
  if (active) y[ooff + m] = (float)acc;
}

// I0(x) by its power series sum_k ((x/2)^2)^k / (k!)^2, summed until a term no longer changes the sum
long double bessel_i0(long double x) {
  const long double y = x * x / 4.0L;
  long double term = 1.0L, sum = 1.0L;
  for (int k = 1; k < 1000; ++k) {
    term *= y / ((long double)k * (long double)k);
    const long double s = sum + term;
    if (s == sum) break;
    sum = s;
  }
  return sum;
}

int check_filter(int32_t up, int32_t down, int32_t zeros, double beta, const char* who) {
  VN_REQUIRE(up > 0 && down > 0, "%s: up=%d, down=%d: both must be positive", who, up, down);
  if (up > RS_MAX_RATIO || down > RS_MAX_RATIO) {
    vaenmf_set_error("%s: ratio %d/%d: this build resamples with up and down of at most %d", who, up, down, RS_MAX_RATIO);
    return RS_NOT_SUPPORTED;
  }
  VN_REQUIRE(zeros >= 1 && zeros <= RS_MAX_ZEROS, "%s: zeros=%d outside [1, %d]", who, zeros, RS_MAX_ZEROS);
  VN_REQUIRE(beta >= 0.0 && beta <= 100.0, "%s: beta=%g outside [0, 100]", who, beta);
  return 0;
}

// h [2 half + 1], natural order; the upper half mirrors the lower bit for bit
void build_taps(int up, int down, int zeros, double beta, double* h) {
  const long double pi = 3.14159265358979323846264338327950288L;
  const int M = up > down ? up : down, half = zeros * M;
  std::vector<long double> v(half + 1);                  // s w at t = 0 .. half
  const long double i0b = bessel_i0((long double)beta);
  long double sum = 0.0L;
  for (int t = half; t >= 0; --t) {                      // small terms first
    long double s = 1.0L / M;
    if (t) {
      int r = t % (2 * M);                               // sin(pi t / M) with the angle reduced to (-pi, pi]
      if (r > M) r -= 2 * M;
      s = sinl(pi * (long double)r / M) / (pi * (long double)t);
    }
    const long double e = (long double)t / half;
    v[t] = s * bessel_i0((long double)beta * sqrtl(1.0L - e * e)) / i0b;
    sum += t ? 2.0L * v[t] : v[t];
  }
  for (int t = 0; t <= half; ++t) h[half + t] = h[half - t] = (double)((long double)up * v[t] / sum);
}

struct TapKey {
  int dev, up, down, zeros;
  double beta;
  bool operator<(const TapKey& o) const { return std::tie(dev, up, down, zeros, beta) < std::tie(o.dev, o.up, o.down, o.zeros, o.beta); }
};

// The polyphase table of one filter on the current device, built on first use (one upload) and kept for the life of the process
int get_taps(int up, int down, int zeros, double beta, ResampleArgs* out) {
  static std::mutex mu;
  static std::map<TapKey, ResampleArgs> tables;
  int dev = 0;
  VN_CHECK_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  const TapKey key{dev, up, down, zeros, beta};
  auto it = tables.find(key);
  if (it == tables.end()) {
    ResampleArgs a{};
    a.up = up; a.down = down;
    a.half = zeros * (up > down ? up : down);
    a.J = (2 * a.half + up) / up;                        // ceil((2 half + 1) / up)
    std::vector<double> h(2 * (size_t)a.half + 1), t((size_t)up * a.J, 0.0);
    build_taps(up, down, zeros, beta, h.data());
    for (int p = 0; p < up; ++p)
      for (int j = 0; p + (int64_t)j * up <= 2 * (int64_t)a.half; ++j) t[(size_t)p * a.J + (a.J - 1 - j)] = h[p + (size_t)j * up];
    double* d = nullptr;
    VN_CHECK_HIP(hipMalloc(&d, t.size() * sizeof(double)));
    const hipError_t ec = hipMemcpy(d, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice);
    if (ec != hipSuccess) {
      (void)hipFree(d);
      VN_CHECK_HIP(ec);
    }
    a.tab = d;
    it = tables.emplace(key, a).first;
  }
  *out = it->second;
  return 0;
}

// Device tables of one batch shape: the offsets and, per workgroup, its utterance and its first output sample
struct BatchTables {
  int dev, up, down;
  std::vector<int64_t> in_off;       // the key: offsets as the caller gave them (the output offsets follow from them)
  int64_t out0;
  char* mem;
  const int64_t *d_in, *d_out, *d_m0;
  const int32_t* d_utt;
  int64_t n_blocks;
  uint64_t used;
};

constexpr size_t RS_BATCH_SHAPES = 16;                   // shapes kept; the least recently used one goes first

int get_batch_tables(int32_t n_utt, const int64_t* in_off, const int64_t* out_off, int up, int down, BatchTables* out) {
  static std::mutex mu;
  static std::vector<BatchTables> cache;
  static uint64_t tick = 0;
  int dev = 0;
  VN_CHECK_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  for (BatchTables& b : cache)
    if (b.dev == dev && b.up == up && b.down == down && b.out0 == out_off[0] && b.in_off.size() == (size_t)n_utt + 1 &&
        std::equal(b.in_off.begin(), b.in_off.end(), in_off)) {
      b.used = ++tick;
      *out = b;
      return 0;
    }
  std::vector<int32_t> utt;
  std::vector<int64_t> m0;
  for (int32_t u = 0; u < n_utt; ++u)
    for (int64_t m = 0; m < out_off[u + 1] - out_off[u]; m += RS_BLOCK) { utt.push_back(u); m0.push_back(m); }
  VN_REQUIRE(utt.size() <= 0x7fffffffu, "vaenmf_resample_batch: %zu workgroups exceed the grid limit", utt.size());
  // byte layout: in_off [n_utt+1] | out_off [n_utt+1] | m0 [nb] | utt [nb]
  const size_t no = (size_t)n_utt + 1, nb = utt.size(), bytes = 8 * (2 * no + nb) + 4 * nb;
  std::vector<char> h(bytes);
  memcpy(h.data(), in_off, 8 * no);
  memcpy(h.data() + 8 * no, out_off, 8 * no);
  memcpy(h.data() + 16 * no, m0.data(), 8 * nb);
  memcpy(h.data() + 16 * no + 8 * nb, utt.data(), 4 * nb);
  BatchTables b{};
  b.dev = dev; b.up = up; b.down = down; b.out0 = out_off[0];
  b.in_off.assign(in_off, in_off + no);
  VN_CHECK_HIP(hipMalloc(&b.mem, bytes));
  const hipError_t ec = hipMemcpy(b.mem, h.data(), bytes, hipMemcpyHostToDevice);
  if (ec != hipSuccess) {
    (void)hipFree(b.mem);
    VN_CHECK_HIP(ec);
  }
  b.d_in = reinterpret_cast<const int64_t*>(b.mem);
  b.d_out = b.d_in + no;
  b.d_m0 = b.d_out + no;
  b.d_utt = reinterpret_cast<const int32_t*>(b.d_m0 + nb);
  b.n_blocks = (int64_t)nb;
  b.used = ++tick;
  if (cache.size() >= RS_BATCH_SHAPES) {
    size_t lru = 0;
    for (size_t i = 1; i < cache.size(); ++i)
      if (cache[i].used < cache[lru].used) lru = i;
    VN_CHECK_HIP(hipFree(cache[lru].mem));              // waits for the launches that still read it
    cache.erase(cache.begin() + lru);
  }
  cache.push_back(b);
  *out = b;
  return 0;
}

int64_t gcd64(int64_t a, int64_t b) {
  while (b) { const int64_t t = a % b; a = b; b = t; }
  return a;
}

}  // namespace

extern "C" int vaenmf_resample_ratio(int64_t fs_in, int64_t fs_out, int32_t* up, int32_t* down) {
  VN_REQUIRE(up && down, "vaenmf_resample_ratio: bad arguments");
  VN_REQUIRE(fs_in > 0 && fs_out > 0, "vaenmf_resample_ratio: rates %lld -> %lld Hz: both must be positive", (long long)fs_in,
             (long long)fs_out);
  const int64_t g = gcd64(fs_in, fs_out), u = fs_out / g, d = fs_in / g;
  if (u > RS_MAX_RATIO || d > RS_MAX_RATIO) {
    vaenmf_set_error("vaenmf_resample_ratio: %lld -> %lld Hz reduces to %lld/%lld: this build resamples with up and down of at most %d",
                     (long long)fs_in, (long long)fs_out, (long long)u, (long long)d, RS_MAX_RATIO);
    return RS_NOT_SUPPORTED;
  }
  *up = (int32_t)u; *down = (int32_t)d;
  return 0;
}

extern "C" int64_t vaenmf_resample_length(int64_t n_in, int32_t up, int32_t down) {
  if (n_in < 0 || up <= 0 || down <= 0) {
    vaenmf_set_error("vaenmf_resample_length: n_in=%lld, up=%d, down=%d", (long long)n_in, up, down);
    return -1;
  }
  const __int128 n = (__int128)n_in * up + down - 1;
  if (n / down > (__int128)INT64_MAX) {
    vaenmf_set_error("vaenmf_resample_length: %lld samples times %d/%d exceed 64 bits", (long long)n_in, up, down);
    return -1;
  }
  return (int64_t)(n / down);
}

extern "C" int vaenmf_resample_taps(int32_t up, int32_t down, int32_t zeros, double beta, double* h) {
  VN_REQUIRE(h, "vaenmf_resample_taps: bad arguments");
  if (int rc = check_filter(up, down, zeros, beta, "vaenmf_resample_taps")) return rc;
  build_taps(up, down, zeros, beta, h);
  return 0;
}

extern "C" int vaenmf_resample_batch(const float* x, int32_t n_utt, const int64_t* in_offsets, const int64_t* out_offsets,
                                     int32_t up, int32_t down, int32_t zeros, double beta, float* y, void* stream) {
  VN_REQUIRE(n_utt >= 0 && up > 0 && down > 0, "vaenmf_resample_batch: n_utt=%d, up=%d, down=%d", n_utt, up, down);
  const int g = (int)gcd64(up, down);
  up /= g; down /= g;
  if (int rc = check_filter(up, down, zeros, beta, "vaenmf_resample_batch")) return rc;
  if (n_utt == 0) return 0;
  VN_REQUIRE(in_offsets && out_offsets, "vaenmf_resample_batch: null offsets");
  for (int32_t u = 0; u < n_utt; ++u) {
    const int64_t n_in = in_offsets[u + 1] - in_offsets[u], n_out = out_offsets[u + 1] - out_offsets[u];
    VN_REQUIRE(n_in >= 0, "vaenmf_resample_batch: in_offsets decrease at utterance %d", u);
    const int64_t want = vaenmf_resample_length(n_in, up, down);
    if (want < 0) return -1;
    VN_REQUIRE(n_out == want, "vaenmf_resample_batch: out_offsets give utterance %d %lld samples, %lld samples at %d/%d are %lld",
               u, (long long)n_out, (long long)n_in, up, down, (long long)want);
  }
  const int64_t total = out_offsets[n_utt] - out_offsets[0];
  if (total == 0) return 0;
  VN_REQUIRE(x && y, "vaenmf_resample_batch: null buffers");
  hipStream_t st = (hipStream_t)stream;
  if (up == down) {                                      // 1/1: the utterances' lengths agree, so one copy moves them all
    VN_CHECK_HIP(hipMemcpyAsync(y + out_offsets[0], x + in_offsets[0], (size_t)total * sizeof(float), hipMemcpyDeviceToDevice, st));
    return 0;
  }
  ResampleArgs a;
  if (int rc = get_taps(up, down, zeros, beta, &a)) return rc;
  BatchTables b;
  if (int rc = get_batch_tables(n_utt, in_offsets, out_offsets, up, down, &b)) return rc;
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)b.n_blocks), dim3(RS_BLOCK), 0, st, x, b.d_in, b.d_out, b.d_utt, b.d_m0, a, y);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}
