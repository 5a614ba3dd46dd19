// volume_kernels.h -- launch wrappers of volume_kernels.hip: the truncated-signed-distance volume of a context (include/flame_nltgv2.h,
// flame_nltgv2_volume_create): fill, fold one inverse-depth map into it, render it into a pinhole camera; and of
// volume_shift_kernels.hip: move the window over the grid (flame_nltgv2_volume_shift_begin).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace flame_hip {

constexpr int kVolumeBlock = 256;  // voxels (pixels) per workgroup and round of every kernel here
constexpr int kIntegrateGrid = 1024;  // the integration's workgroups at most: each walks the volume in strides of the grid
// The counters of a stage lie on the device in kVolumeCountSlots partial sets, kVolumeCountSlotWords ints (one 128-byte line) apart; a
// workgroup adds into set blockIdx % kVolumeCountSlots and the host sums the sets.  One set for all workgroups was measured: 65 536
// workgroups x up to six integer atomics on ONE line took 650 of the 745 us of an integration into 256^3 voxels (profiles/volume.txt).
constexpr int kVolumeCountSlots = 16, kVolumeCountSlotWords = 32;
constexpr size_t kVolumeCountsBytes = sizeof(int) * kVolumeCountSlots * kVolumeCountSlotWords;

// One voxel as it lies on the device, at linear index (k * ny + j) * nx + i.
struct Voxel {
  float tsdf, weight;
};

// The volume's geometry (flame_nltgv2_volume_params).
struct VolumeGrid {
  int nx, ny, nz;
  float voxel_size;
  float origin[3];  // the world position of the centre of GLOBAL voxel (0, 0, 0)
  float trunc, max_weight;
  int base[3];      // local voxel (i, j, k) is global voxel base + (i, j, k): the window (flame_nltgv2_volume_shift_begin)
};

// Per integration call, prepared on the host.
struct IntegrateArgs {
  float K[9];      // row-major
  float pose[12];  // T_cam_world, row-major [R | t]
  int rows, cols;
  float weight, near_depth, min_depth, max_depth;
};

// The counters of an integration as they lie on the device and in pinned memory: flame_nltgv2_integrate_counts.
struct IntegrateCounts {
  int front, in_image, valid, behind, updated, saturated, reserved[2];
};
constexpr int kIntegrateCounters = 6;

// Per raycast call, prepared on the host.
struct RaycastArgs {
  float Kinv[9];   // row-major
  float pose[12];  // T_world_cam, row-major [R | t]
  int rows, cols;
  float z_near, dz;
  int n_steps;
};

// flame_nltgv2_raycast_counts.
struct RaycastCounts {
  int hits, back, empty, reserved;
};

// flame_nltgv2_shift_counts.
struct ShiftCounts {
  int kept, kept_seen, lost_seen, entered, reserved[4];
};
constexpr int kShiftCounters = 4;

inline long volume_blocks(long n) { return (n + kVolumeBlock - 1) / kVolumeBlock; }

// Every voxel {1.0f, 0.0f}.
int launch_volume_fill(const VolumeGrid& g, Voxel* vol, hipStream_t s);

// `map` ([rows * cols] inverse depths) seen from a.pose folded into the volume; counts: kVolumeCountsBytes, cleared first, the partial
// sets of IntegrateCounts.
int launch_volume_integrate(const VolumeGrid& g, const IntegrateArgs& a, const float* map, Voxel* vol, int* counts, hipStream_t s);

// The volume seen from a.pose as an inverse-depth map ([rows * cols], holes the quiet NaN); counts: kVolumeCountsBytes, cleared first,
// the partial sets of RaycastCounts.
int launch_volume_raycast(const VolumeGrid& g, const RaycastArgs& a, const Voxel* vol, float* out, int* counts, hipStream_t s);

// The window moved by `shift` voxels (each |shift[a]| <= n_axis; == n_axis: nothing is kept), out of place: dst[(i, j, k)] =
// src[(i, j, k) + shift] where that lies in the volume, else {1.0f, 0.0f}; src and dst are two buffers of the volume's size, 16-byte
// aligned.  dst == nullptr: nothing is written, only the counters are made (a zero shift).  counts: kVolumeCountsBytes, cleared first,
// the partial sets of ShiftCounts.  -> the bytes per access of the path taken (16 where nx and the linear displacement are even, else 8)
// in *record_bytes.
int launch_volume_shift(const VolumeGrid& g, const int shift[3], const Voxel* src, Voxel* dst, int* counts, int* record_bytes, hipStream_t s);

}  // namespace flame_hip
