// BayesRays, consumer side (fruit_nerf/bayesrays/output_uncertainty.py, bayesrays/utils.py): Hessian grid -> uncertainty table,
// per-sample log uncertainty (+ the density mask), composited uncertainty image.
//   cn_uncertainty_table      elementwise, once per model: streams (L + 1)^3 floats in and out.
//   cn_uncertainty_lookup     one thread per sample: 28 B of ray / sample inputs (the ray's six floats are shared by its samples),
//                             eight 4-byte gathers from the table, 4 B out (+ 8 B for the mask).  The eight addresses of a
//                             sample fall into four 8-byte (z, z + 1) pairs, L and L^2 floats apart.
//   cn_uncertainty_composite  one wavefront per ray, HBM-streaming: 8 B per sample in, 4 B per ray out.
#include "cn_common.hpp"
#include "wave_ops.hpp"

namespace cn {

constexpr float UNC_MIN = -3.f, UNC_MAX = 6.f;  // output_uncertainty.py:41-42

__global__ void __launch_bounds__(256)
uncertainty_table_kernel(const float* __restrict__ hessian, long long n, float N, float reg_lambda, float* __restrict__ un) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += stride)
    un[i] = 1.f / (hessian[i] / N + reg_lambda);
}

__global__ void __launch_bounds__(256)
uncertainty_lookup_kernel(const float* __restrict__ origins, const float* __restrict__ directions,
                          const float* __restrict__ starts, const float* __restrict__ ends, long long total, int S, SceneDev sc,
                          const float* __restrict__ un, unsigned L, float* __restrict__ un_points, float* __restrict__ density,
                          float filter_value) {
  const float Lf = (float)L;
  const unsigned L2 = L * L;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += stride) {
    const long long r = i / S;
    const float mid = (starts[i] + ends[i]) / 2.f;
    float px = origins[3 * r] + directions[3 * r] * mid;
    float py = origins[3 * r + 1] + directions[3 * r + 1] * mid;
    float pz = origins[3 * r + 2] + directions[3 * r + 2] * mid;
    normalize_position(sc, px, py, pz);  // in (0, 1)^3, or zeroed (zero_out=False: such a sample reads vertex 0)
    const float x = px * Lf, y = py * Lf, z = pz * Lf;  // < L: L is a power of two and p < 1
    const float fx = floorf(x), fy = floorf(y), fz = floorf(z);
    // corner c in {0, 1} of an axis: |x - (floor(x) + 1 - c)|
    const float wx[2] = {fabsf(x - (fx + 1.f)), fabsf(x - fx)};
    const float wy[2] = {fabsf(y - (fy + 1.f)), fabsf(y - fy)};
    const float wz[2] = {fabsf(z - (fz + 1.f)), fabsf(z - fz)};
    const unsigned base = (unsigned)(int)fx * L2 + (unsigned)(int)fy * L + (unsigned)(int)fz;  // <= L^3 - 1
    float u[8], c2[8];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {  // k = 4 cx + 2 cy + cz, the reference's corner order
      const int cx = k >> 2, cy = (k >> 1) & 1, cz = k & 1;
      u[k] = un[base + (cx ? L2 : 0u) + (cy ? L : 0u) + (unsigned)cz];  // <= L^3 + L^2 + L < (L + 1)^3
      const float c = wx[cx] * wy[cy] * wz[cz];
      c2[k] = c * c;
      sum += c2[k];
    }
    float acc = 0.f;  // sum >= 1/8: the two coefficients of an axis add up to 1
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += u[k] * (c2[k] / sum);
    const float v = log10f(sqrtf(acc) + 1e-12f);
    un_points[i] = v;
    if (density) density[i] = v <= filter_value ? density[i] : 0.f * density[i];
  }
}

__global__ void __launch_bounds__(256)
uncertainty_composite_kernel(const float* __restrict__ weights, const float* __restrict__ un_points, long long num_rays, int S,
                             float* __restrict__ uncertainty) {
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
  for (long long r = blockIdx.x * (long long)(blockDim.x >> 6) + wave; r < num_rays; r += waves) {
    const long long base = r * (long long)S;
    float sw = 0.f, su = 0.f;
    for (int i = lane; i < S; i += 64) {
      const float w = weights[base + i];
      sw += w;
      su += w * un_points[base + i];
    }
    sw = wave_sum(sw);
    su = wave_sum(su);
    float v = su + (1.f - sw) * UNC_MIN;  // alpha blending against the lower bound
    v = fminf(fmaxf(v, UNC_MIN), UNC_MAX);
    if (lane == 0) uncertainty[r] = (v - UNC_MIN) / (UNC_MAX - UNC_MIN);
  }
}

}  // namespace cn

static int check_lod(int32_t lod, const char* who) {
  // indices and the table size stay below 2^31: (2^10 + 1)^3 = 1 076 890 625
  CN_REQUIRE(lod >= 1 && lod <= 10, CN_ERR_UNSUPPORTED, "%s: lod %d outside [1, 10]", who, lod);
  return CN_OK;
}

extern "C" int cn_uncertainty_table(const float* hessian, int32_t lod, double N, float* un, cn_stream_t stream) {
  CN_REQUIRE(hessian && un, CN_ERR_INVALID, "cn_uncertainty_table: null hessian/un");
  if (int rc = check_lod(lod, "cn_uncertainty_table")) return rc;
  CN_REQUIRE(N > 0.0, CN_ERR_INVALID, "cn_uncertainty_table: N must be > 0");
  const long long L = 1ll << lod, n = (L + 1) * (L + 1) * (L + 1);
  const float reg_lambda = (float)(1e-4 / (double)(L * L * L));
  hipLaunchKernelGGL(cn::uncertainty_table_kernel, dim3(cn::grid_for(n, 256, 8192)), dim3(256), 0, cn::as_stream(stream),
                     hessian, n, (float)N, reg_lambda, un);
  return cn::check_launch("cn_uncertainty_table");
}

extern "C" int cn_uncertainty_lookup(const float* origins, const float* directions, const float* starts, const float* ends,
                                     int64_t num_rays, int32_t num_samples, const cn_scene* scene, const float* un,
                                     int32_t lod, float* un_points, float* density, float filter_value,
                                     cn_stream_t stream) {
  CN_REQUIRE(origins && directions && starts && ends && scene && un && un_points, CN_ERR_INVALID,
             "cn_uncertainty_lookup: null origins/directions/starts/ends/scene/un/un_points");
  CN_REQUIRE(num_samples > 0, CN_ERR_INVALID, "cn_uncertainty_lookup: num_samples must be > 0");
  if (int rc = check_lod(lod, "cn_uncertainty_lookup")) return rc;
  const unsigned long long L = 1ull << lod;
  // a normalised coordinate is < 1, so floor(coord * L) <= L - 1 on every axis and the largest literal index is
  // (L - 1 + 1) L^2 + (L - 1 + 1) L + (L - 1 + 1)
  CN_REQUIRE(L * L * L + L * L + L < (L + 1) * (L + 1) * (L + 1), CN_ERR_INVALID,
             "cn_uncertainty_lookup: corner indices leave the table at lod %d", lod);
  if (num_rays <= 0) return CN_OK;
  const long long total = (long long)num_rays * num_samples;
  hipLaunchKernelGGL(cn::uncertainty_lookup_kernel, dim3(cn::grid_for(total, 256, 1 << 16)), dim3(256), 0,
                     cn::as_stream(stream), origins, directions, starts, ends, total, num_samples, cn::make_scene_dev(*scene),
                     un, (unsigned)L, un_points, density, filter_value);
  return cn::check_launch("cn_uncertainty_lookup");
}

extern "C" int cn_uncertainty_composite(const float* weights, const float* un_points, int64_t num_rays, int32_t num_samples,
                                        float* uncertainty, cn_stream_t stream) {
  CN_REQUIRE(weights && un_points && uncertainty, CN_ERR_INVALID, "cn_uncertainty_composite: null weights/un_points/uncertainty");
  CN_REQUIRE(num_samples > 0, CN_ERR_INVALID, "cn_uncertainty_composite: num_samples must be > 0");
  if (num_rays <= 0) return CN_OK;
  hipLaunchKernelGGL(cn::uncertainty_composite_kernel, dim3(cn::grid_for(num_rays, 4, 16384)), dim3(256), 0,
                     cn::as_stream(stream), weights, un_points, (long long)num_rays, num_samples, uncertainty);
  return cn::check_launch("cn_uncertainty_composite");
}
