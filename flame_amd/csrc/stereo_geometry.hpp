// stereo_geometry.hpp -- the EpipolarGeometry<float> pieces (src/flame/stereo/epipolar_geometry.h) that more than one
// kernel file runs: maxDepthProjection, project(u, idepth, &u_cmp, &new_idepth), referenceEpiline, and cv::Rect::contains.  Used by
// stereo_kernels.hip (updateFeatureIDepths) and feature_kernels.hip (projectFeatures, detectFeatures).  Same
// expression order as the reference and, with the build's -ffp-contract=off, the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "stereo_kernels.h"

namespace flame_hip {

// maxDepthProjection h:191-201
__device__ __forceinline__ V2 max_depth_projection(const Geo& g, V2 u) {
  const float h0 = (g.M[0] * u.x + g.M[1] * u.y) + g.M[2] * 1.0f;
  const float h1 = (g.M[3] * u.x + g.M[4] * u.y) + g.M[5] * 1.0f;
  const float h2 = (g.M[6] * u.x + g.M[7] * u.y) + g.M[8] * 1.0f;
  const float inv = 1.0f / h2;
  return {h0 * inv, h1 * inv};
}

// project(u_ref, idepth, &u_cmp, &new_idepth) h:152-180
__device__ __forceinline__ bool project_idepth(const Geo& g, const StereoCamera& cam, V2 u, float idepth, V2* out,
                                               float* new_idepth) {
  if (!(idepth >= 0.0f)) return false;
  if (idepth == 0.0f) {
    *out = max_depth_projection(g, u);
    *new_idepth = 0.0f;
    return true;
  }
  const float depth = 1.0f / idepth;
  V3 p = {cam.Kinv[0] * u.x + cam.Kinv[2], cam.Kinv[4] * u.y + cam.Kinv[5], 1.0f};
  p.x *= depth, p.y *= depth, p.z *= depth;
  const V3 r = rotate(g.q, p);
  const V3 pc = {r.x + g.t.x, r.y + g.t.y, r.z + g.t.z};
  const float u0 = cam.K[0] * pc.x + cam.K[2] * pc.z;
  const float u1 = cam.K[4] * pc.y + cam.K[5] * pc.z;
  if (!(fabsf(pc.z) > 0.0f)) return false;
  const float nid = 1.0f / pc.z;
  *new_idepth = nid;
  *out = {u0 * nid, u1 * nid};
  return true;
}

// cv::Rect::contains(Point2f): the point becomes a Point2i through cvRound (round to nearest, ties to even) before
// x <= p.x < x + w.  Unpinned reading (OpenCV is not available to check it); shared by the update kernel's move to the
// newest pose-frame and by prunePoseFrames.  A NaN coordinate converts to 0 here (INT_MIN in cvRound on x86): outside
// either way, as the rectangle starts at border >= 1.
__device__ __forceinline__ bool rect_contains(int rx, int ry, int rw, int rh, V2 p) {
  const int ix = __float2int_rn(p.x), iy = __float2int_rn(p.y);
  return rx <= ix && ix < rx + rw && ry <= iy && iy < ry + rh;
}

// referenceEpiline h:303-325
__device__ __forceinline__ bool reference_epiline(const Geo& g, const StereoCamera& cam, V2 u, V2* epi) {
  V2 e = {-cam.K[0] * g.tcr.x + g.tcr.z * (u.x - cam.K[2]), -cam.K[4] * g.tcr.y + g.tcr.z * (u.y - cam.K[5])};
  const float n2 = e.x * e.x + e.y * e.y;
  if (!(n2 > 0)) return false;
  const float inv = (float)(1.0 / sqrt((double)n2));
  e.x *= inv, e.y *= inv;
  *epi = e;
  return true;
}

}  // namespace flame_hip
