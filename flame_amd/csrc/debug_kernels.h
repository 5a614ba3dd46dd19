// debug_kernels.h -- launch wrappers of debug_kernels.hip: the debug images of Flame::update()'s last block, "Draw stuff"
// (flame.cc:490-511) and of drawFeatures (flame.cc:2459-2510), from what already stands on the device
// (include/flame_nltgv2.h, flame_nltgv2_debug_images_begin; include/flame_stereo.h, flame_stereo_draw_features).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace flame_hip {

// Per call, prepared on the host.
struct DebugImageArgs {
  int rows, cols;
  const uint8_t* gray;      // fnew_->img[0]: rows of cols bytes, gray_step bytes apart (device memory)
  int gray_step;
  float scene_color_scale;
  int flip;                 // cv::flip(img, img, -1): the unflipped image in reversed linear pixel order
  float k00, k11;           // K(0,0), K(1,1): what planeParamToNormal reads (flame.cc:2647-2654)
};

// w1_map_ / w2_map_ (flame.cc:498-503) from the rasteriser's key image: the winning triangle of a pixel is the same for every
// attribute, so its index (high word of the key) is taken and the three edge functions are evaluated once more.  `keys` must be the
// key image of a rasterisation of `tris` over `vtx` with every triangle valid.
int launch_debug_wmaps(const unsigned long long* keys, const int32_t* tris, const float2* vtx, const float* w1, const float* w2,
                       float* w1_map, float* w2_map, int rows, int cols, hipStream_t s);

// drawInverseDepthMap (idepth_img != NULL) and drawNormals (normals_img != NULL; reads w1_map / w2_map) over `idepthmap`.
// Images: rows * cols * 3 bytes, 4-byte aligned.
int launch_debug_images(const DebugImageArgs& a, const float* idepthmap, const float* w1_map, const float* w2_map,
                        uint8_t* idepth_img, uint8_t* normals_img, hipStream_t s);

// drawFeatures over n records of `stride_bytes` each, whose first floats at `xy_mu_var` are x, y, idepth_mu, idepth_var.
// owner: rows * cols words of scratch; counts: {num_converged, num_unconverged}.
int launch_draw_features(const DebugImageArgs& a, int n, const void* xy_mu_var, int stride_bytes, float idepth_var_max_graph,
                         uint32_t* owner, int* counts, uint8_t* img, hipStream_t s);

}  // namespace flame_hip
