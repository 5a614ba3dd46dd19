// fuse_kernels.hip -- the kept-mesh snapshot and the fusion of up to eight meshes in one target camera (include/flame_nltgv2.h,
// flame_nltgv2_keep_mesh and flame_nltgv2_fuse_views_begin, state every rule; tests/fuse_ref.py restates them over tests/view_ref.py
// and is the checker, bit for bit):
//   keep        pos and x * scale of the resident mesh into a slot: one float32 multiply per vertex
//   clear       the N key layers, the counters and the big list's count
//   vertices    ONE launch for the vertices of all sources: a lane finds its source by comparing its index with at most eight prefix
//               sums (a source boundary may fall anywhere inside a workgroup), then rule 1 of the view renderer with that source's camera
//   triangles   ONE count launch (rule 2 per triangle; triangles with large boxes listed as (source, triangle) pairs), ONE raster launch
//               (a wavefront per triangle; a block's source is uniform), ONE launch for the listed boxes.  Layer s: keys + s * rows * cols
//   vote        one lane per pixel, 2048-pixel tiles: the N keys are read directly (no resolve pass); the upper median by rank counting
//               over a compile-time 8 (or 1, 2, 4 where fewer sources are named) with presence predicates -- no array is indexed by a
//               run-time value, nothing goes to scratch (profiles/fuse_views.txt has the compiler's resource report); inliers, the weighted mean left to right, masks, spread;
//               the counters through ballot + popcount per wave, LDS per workgroup, one global atomic per non-zero counter
// clear, vertices and the three triangle kernels are thin instances of the bodies in view_project.hpp, which view_kernels.hip
// instantiates for its one source: here the sources are the FuseTable, and of rule 2's classes the drawn one alone is published (word
// 26 of FuseCounts).  keep and vote are this file's own.
// The source table travels by value in the kernel arguments.  No floating-point atomics: two calls give the same bytes.  Built with
// -ffp-contract=off (no FMA); division is correctly rounded.
#include <hip/hip_runtime.h>

#include "fuse_kernels.h"
#include "view_project.hpp"

namespace flame_hip {
namespace {

using namespace view_project;  // the five bodies, shared with view_kernels.hip; FuseTable is this file's model of the sources

constexpr unsigned kHoleBits = 0x7fc00000u;
// words of FuseCounts
constexpr int kWordCoverage = 0, kWordHist = 1, kWordPresent = kWordHist + kFuseSources + 1, kWordInlier = kWordPresent + kFuseSources,
              kWordDrawn = kWordInlier + kFuseSources;
static_assert(kWordDrawn == 26 && offsetof(FuseCounts, tris_drawn) == kWordDrawn * sizeof(int32_t), "the words of FuseCounts");

__global__ void __launch_bounds__(256)
k_keep_vertices(int V, const float2* __restrict__ pos, const float* __restrict__ x, float scale, float2* __restrict__ pos_out,
                float* __restrict__ id_out) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  pos_out[v] = pos[v];
  id_out[v] = x[v] * scale;
}

__global__ void __launch_bounds__(256)
k_fuse_clear(long n, unsigned long long* __restrict__ keys, int* __restrict__ counts, int* __restrict__ big) {
  if (blockIdx.x == 0) {
    if (threadIdx.x < kFuseCountWords) counts[threadIdx.x] = 0;
    if (threadIdx.x == 0) big[0] = 0;
  }
  clear_tile(n, keys);
}

__global__ void __launch_bounds__(256)
k_fuse_vertices(FuseTable tab, ViewVertex* __restrict__ out) { project_vertices(tab, out); }

__global__ void __launch_bounds__(256)
k_fuse_count(FuseTable tab, const ViewVertex* __restrict__ vtx, int* __restrict__ counts, int* __restrict__ big, int rows, int cols) {
  count_triangles(tab, vtx, big, rows, cols, [=](const int* n) { if (n[kDraw]) atomicAdd(&counts[kWordDrawn], n[kDraw]); });
}

__global__ void __launch_bounds__(64)
k_fuse_raster(FuseTable tab, const ViewVertex* __restrict__ vtx, unsigned long long* __restrict__ keys, int rows, int cols) {
  raster_triangle(tab, vtx, keys, rows, cols);
}

__global__ void __launch_bounds__(64)
k_fuse_raster_big(FuseTable tab, const ViewVertex* __restrict__ vtx, const int* __restrict__ big, unsigned long long* __restrict__ keys,
                  int rows, int cols) {
  raster_listed(tab, vtx, big, keys, rows, cols);
}

struct FuseVote {
  float w[kFuseSources];
  int n_sources, min_support;
  float rel_tol;
};

// Rules B - F.  Every loop over the sources has a compile-time trip count and is fully unrolled: b[], pr[], in[] and the wave counters
// are registers, never memory.  kSources: 8, or the next power of two at or above n_sources -- the ranks of one source are no
// comparisons, of eight 56, and at 640x480 the kernel is bound by its instruction stream, not by bytes (profiles/fuse_views.txt).
template <int kSources>
__global__ void __launch_bounds__(256)
k_fuse_vote(FuseVote p, long n, const unsigned long long* __restrict__ keys, FuseOutputs out, int* __restrict__ counts) {
  __shared__ int s_n[kFuseCountWords];
  if (threadIdx.x < kFuseCountWords) s_n[threadIdx.x] = 0;
  __syncthreads();
  int c_cov = 0, c_hist[kSources + 1], c_present[kSources], c_inlier[kSources];
#pragma unroll
  for (int s = 0; s <= kSources; ++s) c_hist[s] = 0;
#pragma unroll
  for (int s = 0; s < kSources; ++s) c_present[s] = c_inlier[s] = 0;
  const long base = (long)blockIdx.x * kViewResolveTile + threadIdx.x;
#pragma unroll 1
  for (int j = 0; j < kPerThread; ++j) {
    const long i = base + (long)j * 256;
    const bool live = i < n;
    unsigned b[kSources];
    bool pr[kSources], in[kSources];
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < kSources; ++s) {
      const unsigned long long k = (live && s < p.n_sources) ? keys[(size_t)s * (size_t)n + (size_t)i] : 0ull;
      pr[s] = (unsigned)k != 0u;  // (the owner's t + 1; 0: nobody)
      b[s] = pr[s] ? (unsigned)(k >> 32) : 0u;
      cnt += pr[s] ? 1 : 0;
    }
    // C: the upper median by rank counting over (bits, source)
    unsigned mbits = 0u;
#pragma unroll
    for (int s = 0; s < kSources; ++s) {
      int rank = 0;
#pragma unroll
      for (int o = 0; o < kSources; ++o) {
        if (o == s) continue;
        rank += (pr[o] && (b[o] < b[s] || (b[o] == b[s] && o < s))) ? 1 : 0;
      }
      if (pr[s] && rank == cnt / 2) mbits = b[s];
    }
    const float m = __uint_as_float(mbits);
    const float tol = p.rel_tol * m;
    // D, E: inliers, and their weighted mean in ascending source index, left to right
    int support = 0;
    float num = 0.0f, den = 0.0f;
    unsigned hi = 0u, lo = 0xffffffffu;
    unsigned pmask = 0u, imask = 0u;
#pragma unroll
    for (int s = 0; s < kSources; ++s) {
      const float v = __uint_as_float(b[s]);
      in[s] = pr[s] && __builtin_fabsf(v - m) <= tol;
      if (in[s]) {
        const float vw = v * p.w[s];
        num = support ? num + vw : vw;
        den = support ? den + p.w[s] : p.w[s];
        ++support;
        hi = b[s] > hi ? b[s] : hi, lo = b[s] < lo ? b[s] : lo;  // (positive floats order as their bits do)
      }
      pmask |= pr[s] ? 1u << s : 0u, imask |= in[s] ? 1u << s : 0u;
    }
    const bool fused = cnt > 0 && support >= p.min_support;
    if (live) {
      if (out.fused) out.fused[i] = fused ? num / den : __uint_as_float(kHoleBits);
      if (out.present_mask) out.present_mask[i] = (uint8_t)pmask;
      if (out.inlier_mask) out.inlier_mask[i] = (uint8_t)imask;
      if (out.spread) out.spread[i] = cnt > 0 ? __uint_as_float(hi) - __uint_as_float(lo) : __uint_as_float(kHoleBits);
      if (out.layers) {
#pragma unroll
        for (int s = 0; s < kSources; ++s)
          if (s < p.n_sources) out.layers[(size_t)s * (size_t)n + (size_t)i] = pr[s] ? __uint_as_float(b[s]) : __uint_as_float(kHoleBits);
      }
    }
    // F: the counters, per wave (every lane of the workgroup arrives at every ballot)
    c_cov += __popcll(__ballot(live && fused));
#pragma unroll
    for (int s = 0; s <= kSources; ++s) c_hist[s] += __popcll(__ballot(live && support == s));
#pragma unroll
    for (int s = 0; s < kSources; ++s) {
      c_present[s] += __popcll(__ballot(pr[s]));  // (a pixel past n has no keys: nothing present)
      c_inlier[s] += __popcll(__ballot(in[s]));
    }
  }
  if ((threadIdx.x & 63) == 0) {
    if (c_cov) atomicAdd(&s_n[kWordCoverage], c_cov);
#pragma unroll
    for (int s = 0; s <= kSources; ++s)
      if (c_hist[s]) atomicAdd(&s_n[kWordHist + s], c_hist[s]);
#pragma unroll
    for (int s = 0; s < kSources; ++s) {
      if (c_present[s]) atomicAdd(&s_n[kWordPresent + s], c_present[s]);
      if (c_inlier[s]) atomicAdd(&s_n[kWordInlier + s], c_inlier[s]);
    }
  }
  __syncthreads();
  if (threadIdx.x < kWordDrawn && s_n[threadIdx.x]) atomicAdd(&counts[threadIdx.x], s_n[threadIdx.x]);
}

}  // namespace

int launch_keep_vertices(int V, const float2* pos, const float* x, float scale, float2* pos_out, float* id_out, hipStream_t s) {
  if (V <= 0) return 0;
  hipLaunchKernelGGL(k_keep_vertices, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, s, V, pos, x, scale, pos_out, id_out);
  return (int)hipGetLastError();
}

int launch_fuse_clear(long n_keys, unsigned long long* keys, FuseCounts* counts, int* big, hipStream_t s) {
  hipLaunchKernelGGL(k_fuse_clear, tiles(n_keys > 0 ? n_keys : 1), dim3(256), 0, s, n_keys, keys, (int*)counts, big);
  return (int)hipGetLastError();
}

int launch_fuse_vertices(const FuseTable& tab, ViewVertex* vtx, hipStream_t s) {
  if (tab.v_end <= 0) return 0;
  hipLaunchKernelGGL(k_fuse_vertices, dim3((unsigned)((tab.v_end + 255) / 256)), dim3(256), 0, s, tab, vtx);
  return (int)hipGetLastError();
}

int launch_fuse_raster(const FuseTable& tab, const ViewVertex* vtx, unsigned long long* keys, FuseCounts* counts, int* big, int rows, int cols,
                       hipStream_t s) {
  if (tab.t_end <= 0) return 0;
  hipLaunchKernelGGL(k_fuse_count, dim3((unsigned)((tab.t_end + 255) / 256)), dim3(256), 0, s, tab, vtx, (int*)counts, big, rows, cols);
  hipLaunchKernelGGL(k_fuse_raster, dim3((unsigned)tab.t_end), dim3(64), 0, s, tab, vtx, keys, rows, cols);
  hipLaunchKernelGGL(k_fuse_raster_big, dim3(kViewBigWaves, kViewBigRows), dim3(64), 0, s, tab, vtx, big, keys, rows, cols);
  return (int)hipGetLastError();
}

int launch_fuse_vote(const FuseTable& tab, long n, const unsigned long long* keys, float rel_tol, int min_support, const FuseOutputs& out,
                     FuseCounts* counts, hipStream_t s) {
  if (n <= 0) return 0;
  FuseVote p;
  for (int k = 0; k < kFuseSources; ++k) p.w[k] = k < tab.n ? tab.s[k].weight : 0.0f;
  p.n_sources = tab.n, p.min_support = min_support, p.rel_tol = rel_tol;
  if (tab.n <= 1) hipLaunchKernelGGL(k_fuse_vote<1>, tiles(n), dim3(256), 0, s, p, n, keys, out, (int*)counts);
  else if (tab.n <= 2) hipLaunchKernelGGL(k_fuse_vote<2>, tiles(n), dim3(256), 0, s, p, n, keys, out, (int*)counts);
  else if (tab.n <= 4) hipLaunchKernelGGL(k_fuse_vote<4>, tiles(n), dim3(256), 0, s, p, n, keys, out, (int*)counts);
  else hipLaunchKernelGGL(k_fuse_vote<kFuseSources>, tiles(n), dim3(256), 0, s, p, n, keys, out, (int*)counts);
  return (int)hipGetLastError();
}

}  // namespace flame_hip
