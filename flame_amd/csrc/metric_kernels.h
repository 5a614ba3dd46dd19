// metric_kernels.h -- launch wrappers of metric_kernels.hip: the metric outputs a consumer of the library reads -- depth image,
// 16-bit millimetre image, organised and dense point cloud, 3-D mesh -- from the maps and the mesh buffers that already stand on the
// device (include/flame_nltgv2.h, flame_nltgv2_metric_outputs_begin).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace flame_hip {

constexpr int kMetricBlock = 256;  // pixels (triangles) per workgroup of every kernel here: one count per workgroup in the scan

// Per call, prepared on the host.
struct MetricArgs {
  int rows, cols;
  float Kinv[9];         // row-major
  float pose[12];        // T_world_cam, row-major [R | t]; read only with has_pose
  int has_pose;
  float min_depth, max_depth;
};

inline long metric_blocks(long n) { return (n + kMetricBlock - 1) / kMetricBlock; }

// One pass over `map` ([rows * cols] inverse depths): depth, depth_mm, organized (each may be NULL) and, with block_count != NULL, the
// number of valid pixels of every workgroup ([metric_blocks(rows * cols)]).
int launch_metric_pixels(const MetricArgs& a, const float* map, float* depth, uint16_t* depth_mm, float* organized, int* block_count,
                         hipStream_t s);

// The ordered compaction behind launch_metric_pixels(block_count): the counts are scanned in place, *n_points is their sum, then every
// valid pixel's point goes to cloud[3 * rank] and its linear index to cloud_pixel[rank], rank = the valid pixels before it in row-major
// order.  No atomics: the result is a function of the map alone.
int launch_metric_cloud(const MetricArgs& a, const float* map, int* block_count, int* n_points, float* cloud, uint32_t* cloud_pixel,
                        hipStream_t s);

// vertices[3v..] = pose(P[v].xyz), normals_out[3v..] = R * normals[3v..]; without a pose both are copied.
int launch_metric_vertices(const MetricArgs& a, int V, const float4* P, const float* normals, float* vertices, float* normals_out,
                           hipStream_t s);

// The index triples of the triangles with tri_valid != 0 in ascending triangle index; *n_valid their number.  block_count:
// [metric_blocks(T)] scratch.
int launch_metric_triangles(int T, const int32_t* tris, const uint8_t* tri_valid, int* block_count, int* n_valid, int32_t* out,
                            hipStream_t s);

}  // namespace flame_hip
