// Views of a labelled point cloud without a window: a z-tested point splat of ONE cloud into F pinhole frames per launch
// (cn_splat_points; the geometry is defined in include/cropnerf_hip.h and restated in float64 by tests/test_splat.py).
//
//   splat_points_kernel    one thread per point, looping over the frames of the launch: the position is read once, the 16
//                          camera floats of a frame are wave-uniform and come through scalar loads (constant address space).
//                          Per covered pixel a 64-bit key -- float32 bits of the camera z in the high word (a positive
//                          float's bits are order-preserving), the point index in the low word -- is merged with atomicMin:
//                          smallest depth wins, equal depths go to the smallest index, whatever order the waves run in.
//                          The pixel's current key is read with a plain load first and the atomic is issued only when the new
//                          key is smaller: in a dense cloud most candidates lose, and a lost atomic is still a read-modify-
//                          write at the L2.  Keys only ever decrease, so a stale value from the L1 can cost a needless atomic
//                          but never hide a winner.  -DCN_SPLAT_NO_PRETEST compiles the load out (tools/splat_probe.py).
//   splat_resolve_kernel   1024 pixels per block: key -> index / depth (coalesced dwords) and the winner's colour or the
//                          background, staged in LDS so that the 3-byte pixels leave as whole dwords.
#include "cn_common.hpp"

namespace cn {

constexpr unsigned long long SPLAT_EMPTY = 0xffffffffffffffffull;  // the high word is a NaN pattern: no point makes it

__global__ void __launch_bounds__(256)
splat_points_kernel(const float* __restrict__ points, long long n, const float* cameras, int num_frames, int H, int W,
                    float half_size, float near_plane, unsigned long long* keys) {
  const cfloat_ptr cam_all = as_const(cameras);
  const float wmax = (float)(W - 1), hmax = (float)(H - 1);
  const size_t frame_pixels = (size_t)H * W;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
    for (int f = 0; f < num_frames; ++f) {
      const cfloat_ptr cam = cam_all + 16 * f;
      const float cz = fmaf(cam[8], x, fmaf(cam[9], y, fmaf(cam[10], z, cam[11])));
      if (!(cz > near_plane)) continue;  // behind the near plane (or not a number)
      const float cx = fmaf(cam[0], x, fmaf(cam[1], y, fmaf(cam[2], z, cam[3])));
      const float cy = fmaf(cam[4], x, fmaf(cam[5], y, fmaf(cam[6], z, cam[7])));
      const float u = fmaf(cam[12], cx / cz, cam[14]), v = fmaf(cam[13], cy / cz, cam[15]);
      // columns ceil(u - s/2) .. ceil(u + s/2) - 1, rows alike; tested and clipped while still float (a huge or not-a-number
      // coordinate must not reach an int, and fminf / fmaxf would turn a NaN into the image's edge)
      const float ja = ceilf(u - half_size), jb = ceilf(u + half_size) - 1.f;
      const float ia = ceilf(v - half_size), ib = ceilf(v + half_size) - 1.f;
      if (!(ja <= wmax && jb >= 0.f && ia <= hmax && ib >= 0.f)) continue;  // entirely outside the image
      const float j0f = fmaxf(ja, 0.f), j1f = fminf(jb, wmax), i0f = fmaxf(ia, 0.f), i1f = fminf(ib, hmax);
      const int j0 = (int)j0f, j1 = (int)j1f, i0 = (int)i0f, i1 = (int)i1f;
      const unsigned long long key = ((unsigned long long)__float_as_uint(cz) << 32) | (unsigned long long)(unsigned)i;
      unsigned long long* frame = keys + (size_t)f * frame_pixels;
      for (int r = i0; r <= i1; ++r) {
        unsigned long long* row = frame + (size_t)r * W;
        for (int c = j0; c <= j1; ++c) {
#if !defined(CN_SPLAT_NO_PRETEST)
          if (key < row[c])
#endif
            atomicMin(row + c, key);
        }
      }
    }
  }
}

constexpr int RESOLVE_PIXELS = 1024;  // per block of 256 threads: 3072 colour bytes = 768 dwords, three per thread

__global__ void __launch_bounds__(256)
splat_resolve_kernel(const unsigned long long* __restrict__ keys, const unsigned char* __restrict__ colors, size_t num_pixels,
                     unsigned background, unsigned char* __restrict__ images, int* __restrict__ index,
                     float* __restrict__ depth) {
  __shared__ unsigned rgb_words[RESOLVE_PIXELS * 3 / 4];
  unsigned char* rgb = reinterpret_cast<unsigned char*>(rgb_words);
  const size_t base = (size_t)blockIdx.x * RESOLVE_PIXELS;
  const unsigned char bg_r = background & 255u, bg_g = (background >> 8) & 255u, bg_b = (background >> 16) & 255u;
#pragma unroll
  for (int k = 0; k < RESOLVE_PIXELS / 256; ++k) {
    const int local = k * 256 + threadIdx.x;
    const size_t p = base + local;
    if (p >= num_pixels) break;
    const unsigned long long key = keys[p];
    const bool hit = key != SPLAT_EMPTY;
    const unsigned point = (unsigned)key;
    unsigned char r = bg_r, g = bg_g, b = bg_b;
    if (hit) {
      const unsigned char* c = colors + 3ull * point;
      r = c[0];
      g = c[1];
      b = c[2];
    }
    rgb[3 * local] = r;
    rgb[3 * local + 1] = g;
    rgb[3 * local + 2] = b;
    if (index) index[p] = hit ? (int)point : -1;
    if (depth) depth[p] = hit ? __uint_as_float((unsigned)(key >> 32)) : __builtin_inff();
  }
  __syncthreads();
  unsigned char* out = images + 3 * base;  // 3072 bytes per block: dword-aligned whenever `images` is
  const bool whole = base + RESOLVE_PIXELS <= num_pixels && (reinterpret_cast<uintptr_t>(images) & 3u) == 0;
  if (whole) {  // block-uniform
    unsigned* out_words = reinterpret_cast<unsigned*>(out);
#pragma unroll
    for (int k = 0; k < 3; ++k) out_words[k * 256 + threadIdx.x] = rgb_words[k * 256 + threadIdx.x];
  } else {
    const size_t left = num_pixels - base;
    const int bytes = 3 * (int)(left < (size_t)RESOLVE_PIXELS ? left : (size_t)RESOLVE_PIXELS);
    for (int t = threadIdx.x; t < bytes; t += 256) out[t] = rgb[t];
  }
}

}  // namespace cn

extern "C" size_t cn_splat_workspace_bytes(int32_t num_frames, int32_t height, int32_t width) {
  return num_frames > 0 && height > 0 && width > 0 ? (size_t)num_frames * height * width * sizeof(unsigned long long) : 0;
}

extern "C" int cn_splat_points(const float* points, const uint8_t* colors, int64_t num_points, const float* cameras,
                               int32_t num_frames, int32_t height, int32_t width, int32_t point_size, float near_plane,
                               uint32_t background_rgb, uint8_t* images, int32_t* index, float* depth, void* workspace,
                               size_t workspace_bytes, cn_stream_t stream) {
  CN_REQUIRE(cameras && images && workspace, CN_ERR_INVALID, "cn_splat_points: null argument");
  CN_REQUIRE(num_points >= 0 && num_points < (1ll << 32), CN_ERR_INVALID,
             "cn_splat_points: %lld points (the key holds a 32-bit index)", (long long)num_points);
  CN_REQUIRE(num_points == 0 || (points && colors), CN_ERR_INVALID, "cn_splat_points: null points or colours");
  CN_REQUIRE(num_frames > 0 && height > 0 && width > 0, CN_ERR_INVALID, "cn_splat_points: bad frame count or image size");
  CN_REQUIRE(point_size >= 1, CN_ERR_INVALID, "cn_splat_points: point_size %d < 1", (int)point_size);
  CN_REQUIRE(near_plane >= 0.f, CN_ERR_INVALID, "cn_splat_points: near_plane must be >= 0 (the depth key is a positive float)");
  const size_t need = cn_splat_workspace_bytes(num_frames, height, width);
  CN_REQUIRE(workspace_bytes >= need, CN_ERR_INVALID, "cn_splat_points: workspace too small (%zu < %zu bytes)",
             workspace_bytes, need);
  hipStream_t s = cn::as_stream(stream);
  unsigned long long* keys = static_cast<unsigned long long*>(workspace);
  const size_t num_pixels = (size_t)num_frames * height * width;
  CN_REQUIRE((num_pixels + cn::RESOLVE_PIXELS - 1) / cn::RESOLVE_PIXELS <= 0x7fffffffull, CN_ERR_INVALID,
             "cn_splat_points: %zu pixels in one launch", num_pixels);
  const hipError_t cleared = hipMemsetAsync(keys, 0xff, need, s);
  CN_REQUIRE(cleared == hipSuccess, CN_ERR_LAUNCH, "cn_splat_points: clearing the keys: %s", hipGetErrorString(cleared));
  if (num_points > 0)
    hipLaunchKernelGGL(cn::splat_points_kernel, dim3(cn::grid_for(num_points, 256)), dim3(256), 0, s, points,
                       (long long)num_points, cameras, (int)num_frames, (int)height, (int)width, 0.5f * (float)point_size,
                       near_plane, keys);
  hipLaunchKernelGGL(cn::splat_resolve_kernel, dim3((unsigned)((num_pixels + cn::RESOLVE_PIXELS - 1) / cn::RESOLVE_PIXELS)),
                     dim3(256), 0, s, keys, colors, num_pixels, (unsigned)background_rgb, images, index, depth);
  return cn::check_launch("cn_splat_points");
}
