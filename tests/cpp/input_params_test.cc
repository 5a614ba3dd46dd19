// The pure host part of the raw-frame input stage (flame_amd/csrc/input_params.hpp): bytes per pixel, the validation that
// flame_stereo_set_input and flame_stereo_add_raw_frame share, the extent of a raw frame and the grid arithmetic of
// k_input_rectify.  Walks formats, sizes and strides: a frame that passes is read over exactly input_frame_bytes() bytes of a
// buffer of exactly that size (under AddressSanitizer when built that way), and the grid covers every output pixel once.
//   input_params_test      exit 0: all held; 1: a violation (printed)
#include <cstdio>
#include <vector>

#include "input_params.hpp"

using namespace flame_hip;

static int bad = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++bad;                                                      \
    }                                                             \
  } while (0)

int main() {
  // bytes per pixel
  const int want_bpp[] = {1, 3, 3, 4, 4};
  for (int f = 0; f < 5; ++f) EXPECT(input_bytes_per_pixel(f) == want_bpp[f]);
  EXPECT(input_bytes_per_pixel(-1) == 0 && input_bytes_per_pixel(5) == 0 && input_bytes_per_pixel(1 << 30) == 0);

  // validation of the parameters
  flame_stereo_input_params p = {};
  p.format = FLAME_STEREO_FMT_BGR8, p.remap = 1, p.raw_width = 67, p.raw_height = 41;
  EXPECT(input_params_valid(&p, 61, 37));
  EXPECT(!input_params_valid(nullptr, 61, 37));
  for (int f : {-1, 5, 99}) {
    flame_stereo_input_params q = p;
    q.format = f;
    EXPECT(!input_params_valid(&q, 61, 37));
  }
  for (int r : {-1, 2}) {
    flame_stereo_input_params q = p;
    q.remap = r;
    EXPECT(!input_params_valid(&q, 61, 37));
  }
  for (int d : {-5, 0, 1, kInputMaxDim + 1}) {
    flame_stereo_input_params q = p;
    q.raw_width = d;
    EXPECT(!input_params_valid(&q, 61, 37));
    q = p;
    q.raw_height = d;
    EXPECT(!input_params_valid(&q, 61, 37));
  }
  {
    flame_stereo_input_params q = p;
    q.remap = 0;
    EXPECT(!input_params_valid(&q, 61, 37));  // remap 0 with another size
    q.raw_width = 61, q.raw_height = 37;
    EXPECT(input_params_valid(&q, 61, 37));
    q.raw_width = kInputMaxDim, q.raw_height = kInputMaxDim;
    EXPECT(input_params_valid(&q, kInputMaxDim, kInputMaxDim));
  }

  // a frame that passes is readable over its whole extent, and no further
  int frames = 0;
  for (int f = 0; f < 5; ++f)
    for (int w : {2, 3, 61, 67})
      for (int h : {2, 5, 41})
        for (int extra : {-1, 0, 1, 5, 64}) {
          flame_stereo_input_params q = p;
          q.format = f, q.raw_width = w, q.raw_height = h;
          const int bpp = input_bytes_per_pixel(f), stride = w * bpp + extra;
          uint8_t one = 0;
          EXPECT(input_frame_valid(q, &one, stride) == (extra >= 0));
          EXPECT(!input_frame_valid(q, nullptr, stride));
          if (extra < 0) continue;
          const size_t bytes = input_frame_bytes(q, stride);
          EXPECT(bytes == (size_t)(h - 1) * stride + (size_t)w * bpp);
          std::vector<uint8_t> buf(bytes, 1);
          unsigned sum = 0;
          for (int y = 0; y < h; ++y)
            for (int x = 0; x < w * bpp; ++x) sum += buf[(size_t)y * stride + x];  // every pixel byte lies inside
          EXPECT(sum == (unsigned)(h * w * bpp));
          ++frames;
        }
  // the largest frame's extent needs more than 32 bits
  {
    flame_stereo_input_params q = p;
    q.format = FLAME_STEREO_FMT_RGBA8, q.raw_width = kInputMaxDim, q.raw_height = kInputMaxDim;
    EXPECT(input_frame_valid(q, &q, 4 * kInputMaxDim) && !input_frame_valid(q, &q, 4 * kInputMaxDim - 1));
    EXPECT(input_frame_bytes(q, 4 * kInputMaxDim) == (size_t)4 * kInputMaxDim * kInputMaxDim);
  }

  // the grid: every pixel owned by exactly one thread, the last thread owns 1..4, the last block is not empty
  int grids = 0;
  for (long n : {1L, 3L, 4L, 5L, 1023L, 1024L, 1025L, 2257L, 61L * 37, 640L * 480, 1920L * 1080, (long)kInputMaxDim * kInputMaxDim}) {
    const long threads = input_threads(n);
    const long blocks = input_blocks(n);
    EXPECT((threads - 1) * kInputPixelsPerThread < n && threads * kInputPixelsPerThread >= n);
    EXPECT((blocks - 1) * kInputBlock < threads && blocks * kInputBlock >= threads);
    EXPECT(blocks * kInputBlock * (long)kInputPixelsPerThread < (1L << 31));  // the kernel's int pixel index
    ++grids;
  }
  std::printf("%d frames and %d grids walked, %d violations\n", frames, grids, bad);
  return bad ? 1 : 0;
}
