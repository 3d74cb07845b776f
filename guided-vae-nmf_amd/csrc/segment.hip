// Long recordings as many short utterances: the segment table (host) and the two row movers around the EM engine (device).
//
// Rule for a recording of n frames, segment length L >= 2, overlap 0 <= V <= L / 2, stride = L - V:
//   m = max(1, floor((n - V) / stride)) segments, segment k starts at frame k stride; segments 0 .. m-2 have L frames, the
//   last one runs to frame n (n frames when m = 1, else L <= length < L + stride).
// Hence a recording of fewer than L + stride frames is one segment, every frame lies in one segment or in two consecutive
// ones, every overlap has exactly V frames, and -- V <= L / 2 -- no frame lies in three.
// Blend weight of the i-th overlap frame (i = 0 .. V-1): later segment w_b = float((i + 1) / (V + 1)) (double, rounded
// once), earlier segment w_a = 1.0f - w_b (float).
// Processing order of the segments of a batch of recordings: first every L-frame segment that is not its recording's last
// (recording order, then segment order: one shape, so that full rounds of them repeat a batch shape), then the recordings'
// last segments in recording order.  Segment rows are numbered in that order.
//
// gather_rows / blend_rows are pure gathers over disjoint output rows (no atomics, no read-modify-write): a frame's value
// does not depend on which round its segments ran in.  A group of `lpr` lanes (a power of two, <= 64) serves one row, so
// that a 64-lane wavefront moves 64 / lpr rows at a time: the row's indices are loaded once per row, then the lanes walk
// the row 16 bytes at a time (row_floats a multiple of 4 and both bases 16-byte aligned) or float by float.
#include <stdint.h>
#include <vector>
#include "common.h"

namespace {

constexpr int SG_BLOCK = 256;
constexpr int SG_MAX_GRID = 2048;     // workgroups at most; the rows beyond are taken grid-stride

typedef float4 Row4;                  // 16 bytes, moved as one

template <typename T> __device__ __forceinline__ T blend2(T a, T b, float wa, float wb);
template <> __device__ __forceinline__ float blend2<float>(float a, float b, float wa, float wb) {
  // two products rounded on their own, then one sum: the same bits whichever operand comes first.  Plain operators under
  // the pragma, not __fmul_rn / __fadd_rn: those are x * y and x + y compiled with the header's contraction setting, and
  // the backend fused them into v_pk_fma_f32 here.
#pragma clang fp contract(off)
  const float pa = wa * a, pb = wb * b;
  return pa + pb;
}
template <> __device__ __forceinline__ Row4 blend2<Row4>(Row4 a, Row4 b, float wa, float wb) {
  return make_float4(blend2(a.x, b.x, wa, wb), blend2(a.y, b.y, wa, wb), blend2(a.z, b.z, wa, wb), blend2(a.w, b.w, wa, wb));
}

// units: elements of T per row; lpr_log2: log2 of the lanes that share a row
template <typename T>
__global__ __launch_bounds__(SG_BLOCK) void gather_rows_kernel(const T* __restrict__ src, const int32_t* __restrict__ row_map,
                                                               int64_t n_rows, int32_t units, int32_t lpr_log2, T* __restrict__ dst) {
  const int lpr = 1 << lpr_log2, rows_per_block = SG_BLOCK >> lpr_log2;
  const int sub = threadIdx.x >> lpr_log2, lane = threadIdx.x & (lpr - 1);
  for (int64_t r = (int64_t)blockIdx.x * rows_per_block + sub; r < n_rows; r += (int64_t)gridDim.x * rows_per_block) {
    const T* __restrict__ s = src + (size_t)row_map[r] * units;
    T* __restrict__ d = dst + (size_t)r * units;
    for (int c = lane; c < units; c += lpr) d[c] = s[c];
  }
}

template <typename T>
__global__ __launch_bounds__(SG_BLOCK) void blend_rows_kernel(const T* __restrict__ seg, const int32_t* __restrict__ row_a,
                                                              const int32_t* __restrict__ row_b, const float* __restrict__ w_b,
                                                              int64_t n_frames, int32_t units, int32_t lpr_log2, T* __restrict__ dst) {
  const int lpr = 1 << lpr_log2, rows_per_block = SG_BLOCK >> lpr_log2;
  const int sub = threadIdx.x >> lpr_log2, lane = threadIdx.x & (lpr - 1);
  for (int64_t t = (int64_t)blockIdx.x * rows_per_block + sub; t < n_frames; t += (int64_t)gridDim.x * rows_per_block) {
    const int32_t ra = row_a[t], rb = row_b[t];
    const T* __restrict__ a = seg + (size_t)ra * units;
    T* __restrict__ d = dst + (size_t)t * units;
    if (rb < 0) {                                                  // one owner: its bits
      for (int c = lane; c < units; c += lpr) d[c] = a[c];
    } else {
      const float wb = w_b[t], wa = __fsub_rn(1.0f, wb);
      const T* __restrict__ b = seg + (size_t)rb * units;
      for (int c = lane; c < units; c += lpr) d[c] = blend2<T>(a[c], b[c], wa, wb);
    }
  }
}

struct RowShape { bool vec; int32_t units, lpr_log2; unsigned grid; };

// 16-byte units when the rows and both bases allow, floats otherwise; the smallest power of two of lanes that covers a row
RowShape row_shape(const void* p0, const void* p1, int64_t n_rows, int32_t row_floats) {
  RowShape s;
  s.vec = row_floats % 4 == 0 && (((uintptr_t)p0 | (uintptr_t)p1) & 15) == 0;
  s.units = s.vec ? row_floats / 4 : row_floats;
  s.lpr_log2 = 0;
  while (s.lpr_log2 < 6 && (1 << s.lpr_log2) < s.units) ++s.lpr_log2;
  const int64_t rows_per_block = SG_BLOCK >> s.lpr_log2, blocks = (n_rows + rows_per_block - 1) / rows_per_block;
  s.grid = (unsigned)(blocks < SG_MAX_GRID ? blocks : SG_MAX_GRID);
  return s;
}

int check_rule(int32_t L, int32_t V, const char* who) {
  VN_REQUIRE(L >= 2, "%s: segment length L=%d frames: at least 2", who, L);
  VN_REQUIRE(V >= 0 && V <= L / 2, "%s: overlap V=%d frames outside [0, L/2 = %d] (L=%d)", who, V, L / 2, L);
  return 0;
}

inline int64_t segments_of(int64_t n, int32_t L, int32_t V) {
  const int64_t stride = L - V, q = n - V;
  return q >= stride ? q / stride : 1;
}

}  // namespace

extern "C" int vaenmf_segment_count(int32_t n_utt, const int32_t* frame_counts, int32_t L, int32_t V, int64_t* n_segments,
                                    int64_t* n_segment_rows) {
  VN_REQUIRE(n_utt >= 0 && (frame_counts || n_utt == 0) && n_segments && n_segment_rows, "vaenmf_segment_count: bad arguments");
  if (int rc = check_rule(L, V, "vaenmf_segment_count")) return rc;
  int64_t segs = 0, rows = 0;
  for (int32_t u = 0; u < n_utt; ++u) {
    const int64_t n = frame_counts[u];
    VN_REQUIRE(n >= 1, "vaenmf_segment_count: recording %d has %lld frames", u, (long long)n);
    const int64_t m = segments_of(n, L, V);
    segs += m;
    rows += n + (m - 1) * V;                              // every seam counts its V frames twice
  }
  *n_segments = segs;
  *n_segment_rows = rows;
  return 0;
}

extern "C" int vaenmf_segment_table(int32_t n_utt, const int32_t* frame_counts, int32_t L, int32_t V, int32_t max_frames,
                                    int32_t* seg_utt, int32_t* seg_index, int32_t* seg_first, int32_t* seg_len,
                                    int32_t* src_row, int32_t* row_a, int32_t* row_b, float* w_b) {
  int64_t n_seg = 0, n_rows = 0;
  if (int rc = vaenmf_segment_count(n_utt, frame_counts, L, V, &n_seg, &n_rows)) return rc;
  const int64_t stride = L - V;
  VN_REQUIRE(L + stride - 1 <= (int64_t)max_frames,
             "vaenmf_segment_table: segments of L=%d frames with overlap V=%d run up to L + stride - 1 = %lld frames, the engine holds max_frames=%d",
             L, V, (long long)(L + stride - 1), max_frames);
  VN_REQUIRE(n_rows <= INT32_MAX, "vaenmf_segment_table: %lld segment rows exceed 32-bit row indices", (long long)n_rows);
  if (n_utt == 0) return 0;
  VN_REQUIRE(seg_utt && seg_index && seg_first && seg_len && src_row && row_a && row_b && w_b, "vaenmf_segment_table: null table");
  // positions in processing order: the L-frame segments of recording u start at g1[u], its last segment is G1 + u
  std::vector<int64_t> g1(n_utt), last_row(n_utt), off(n_utt);
  int64_t G1 = 0, frames = 0;
  for (int32_t u = 0; u < n_utt; ++u) {
    g1[u] = G1;
    off[u] = frames;
    G1 += segments_of(frame_counts[u], L, V) - 1;
    frames += frame_counts[u];
  }
  int64_t row = G1 * L;
  for (int32_t u = 0; u < n_utt; ++u) {
    const int64_t n = frame_counts[u], m = segments_of(n, L, V), len = n - (m - 1) * stride;
    last_row[u] = row;
    for (int64_t j = 0; j < m; ++j) {
      const bool last = j == m - 1;
      const int64_t p = last ? G1 + u : g1[u] + j, r0 = last ? row : p * L, cnt = last ? len : L;
      seg_utt[p] = u;
      seg_index[p] = (int32_t)j;
      seg_first[p] = (int32_t)(j * stride);
      seg_len[p] = (int32_t)cnt;
      for (int64_t i = 0; i < cnt; ++i) src_row[r0 + i] = (int32_t)(off[u] + j * stride + i);
    }
    row += len;
    // owners of frame t: the last segment that starts at or before it, and the one before while t is inside its L frames
    for (int64_t t = 0; t < n; ++t) {
      int64_t j = t / stride;
      if (j > m - 1) j = m - 1;
      const int64_t i = t - j * stride;
      const int64_t rj = (j == m - 1 ? last_row[u] : (g1[u] + j) * L) + i;
      if (j >= 1 && i < V) {
        row_a[off[u] + t] = (int32_t)((g1[u] + j - 1) * L + stride + i);
        row_b[off[u] + t] = (int32_t)rj;
        w_b[off[u] + t] = (float)((double)(i + 1) / (double)(V + 1));
      } else {
        row_a[off[u] + t] = (int32_t)rj;
        row_b[off[u] + t] = -1;
        w_b[off[u] + t] = 0.0f;
      }
    }
  }
  return 0;
}

extern "C" int vaenmf_gather_rows(const float* src, const int32_t* row_map, int64_t n_rows, int32_t row_floats, float* dst,
                                  void* stream) {
  VN_REQUIRE(n_rows >= 0 && row_floats >= 0, "vaenmf_gather_rows: n_rows=%lld, row_floats=%d", (long long)n_rows, row_floats);
  if (n_rows == 0 || row_floats == 0) return 0;
  VN_REQUIRE(src && row_map && dst, "vaenmf_gather_rows: null buffers");
  const RowShape s = row_shape(src, dst, n_rows, row_floats);
  hipStream_t st = (hipStream_t)stream;
  if (s.vec)
    hipLaunchKernelGGL(gather_rows_kernel<Row4>, dim3(s.grid), dim3(SG_BLOCK), 0, st, reinterpret_cast<const Row4*>(src), row_map,
                       n_rows, s.units, s.lpr_log2, reinterpret_cast<Row4*>(dst));
  else
    hipLaunchKernelGGL(gather_rows_kernel<float>, dim3(s.grid), dim3(SG_BLOCK), 0, st, src, row_map, n_rows, s.units, s.lpr_log2, dst);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int vaenmf_blend_rows(const float* seg, const int32_t* row_a, const int32_t* row_b, const float* w_b, int64_t n_frames,
                                 int32_t row_floats, float* dst, void* stream) {
  VN_REQUIRE(n_frames >= 0 && row_floats >= 0, "vaenmf_blend_rows: n_frames=%lld, row_floats=%d", (long long)n_frames, row_floats);
  if (n_frames == 0 || row_floats == 0) return 0;
  VN_REQUIRE(seg && row_a && row_b && w_b && dst, "vaenmf_blend_rows: null buffers");
  const RowShape s = row_shape(seg, dst, n_frames, row_floats);
  hipStream_t st = (hipStream_t)stream;
  if (s.vec)
    hipLaunchKernelGGL(blend_rows_kernel<Row4>, dim3(s.grid), dim3(SG_BLOCK), 0, st, reinterpret_cast<const Row4*>(seg), row_a,
                       row_b, w_b, n_frames, s.units, s.lpr_log2, reinterpret_cast<Row4*>(dst));
  else
    hipLaunchKernelGGL(blend_rows_kernel<float>, dim3(s.grid), dim3(SG_BLOCK), 0, st, seg, row_a, row_b, w_b, n_frames, s.units,
                       s.lpr_log2, dst);
  VN_CHECK_HIP(hipGetLastError());
  return 0;
}
