// BayesRays (fruit_nerf/bayesrays/): the Hessian grid and what is rendered from it.
// Consumer side (output_uncertainty.py, bayesrays/utils.py): Hessian grid -> uncertainty table, per-sample log uncertainty
// (+ the density mask), composited uncertainty image.
//   cn_uncertainty_table      elementwise, once per model: streams (L + 1)^3 floats in and out.
//   cn_uncertainty_lookup     one thread per sample: 28 B of ray / sample inputs (the ray's six floats are shared by its samples),
//                             eight 4-byte gathers from the table, 4 B out (+ 8 B for the mask).  The eight addresses of a
//                             sample fall into four 8-byte (z, z + 1) pairs, L and L^2 floats apart.
//   cn_uncertainty_composite  one wavefront per ray, HBM-streaming: 8 B per sample in, 4 B per ray out.
// Producer side (bayesrays/uncertainty.py:44-90, 292-339): H[v] += 3 |sum_{samples of a ray} coef_v d semantics / d x|^2.
//   cn_semantics_density_gradient       one wavefront per ray, HBM-streaming: 16 B per sample in, 4-8 B out.
//   cn_field_density_position_gradient  one thread per sample: the 128 gathers of the field's grid (the cost: a CU's L1 looks up
//                                       one line per clock), 2 * 2 * 32 * H fp32 multiply-adds (H = 64: 8.2 k flop), 12 B out.
//                                       No parameter gradient, no atomic, no LDS.
//   cn_hessian_accumulate               one wavefront per ray: 8 S (index, coef * g) records merged by index in a per-wave LDS
//                                       hash table, then one float atomic per distinct vertex of the ray.
#include "cn_common.hpp"
#include "wave_ops.hpp"

namespace cn {

constexpr float UNC_MIN = -3.f, UNC_MAX = 6.f;  // output_uncertainty.py:41-42

// find_grid_indices (bayesrays/utils.py:16-41) for a NORMALISED position in [0, 1)^3: the eight literal vertex indices
// (floor(x) + cx) L^2 + (floor(y) + cy) L + (floor(z) + cz) -- stride L in a table of (L + 1)^3, so vertices alias, as in the
// reference -- and their trilinear coefficients |x - (floor(x) + 1 - cx)| ...  Corner k = 4 cx + 2 cy + cz, the reference's order.
// One definition for the table's reader (cn_uncertainty_lookup) and its writer (cn_hessian_accumulate).
struct GridCorners {
  float wx[2], wy[2], wz[2];
  unsigned base;  // <= L^3 - 1: a normalised coordinate is < 1 and L a power of two, so floor(coord * L) <= L - 1
  __device__ __forceinline__ unsigned index(int k, unsigned L) const {  // <= L^3 + L^2 + L < (L + 1)^3
    return base + ((k >> 2) ? L * L : 0u) + (((k >> 1) & 1) ? L : 0u) + (unsigned)(k & 1);
  }
  __device__ __forceinline__ float coef(int k) const { return wx[k >> 2] * wy[(k >> 1) & 1] * wz[k & 1]; }
};
__device__ __forceinline__ GridCorners grid_corners(float px, float py, float pz, unsigned L) {
  const float Lf = (float)L;
  const float x = px * Lf, y = py * Lf, z = pz * Lf;
  const float fx = floorf(x), fy = floorf(y), fz = floorf(z);
  GridCorners g;
  g.wx[0] = fabsf(x - (fx + 1.f));
  g.wx[1] = fabsf(x - fx);
  g.wy[0] = fabsf(y - (fy + 1.f));
  g.wy[1] = fabsf(y - fy);
  g.wz[0] = fabsf(z - (fz + 1.f));
  g.wz[1] = fabsf(z - fz);
  g.base = (unsigned)(int)fx * (L * L) + (unsigned)(int)fy * L + (unsigned)(int)fz;
  return g;
}

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
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += stride) {
    const long long r = i / S;
    const float mid = (starts[i] + ends[i]) / 2.f;
    float px = origins[3 * r] + directions[3 * r] * mid;
    float py = origins[3 * r + 1] + directions[3 * r + 1] * mid;
    float pz = origins[3 * r + 2] + directions[3 * r + 2] * mid;
    normalize_position(sc, px, py, pz);  // in (0, 1)^3, or zeroed (zero_out=False: such a sample reads vertex 0)
    const GridCorners g = grid_corners(px, py, pz, L);
    float u[8], c2[8];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {  // k = 4 cx + 2 cy + cz, the reference's corner order
      u[k] = un[g.index(k, L)];
      const float c = g.coef(k);
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

// ---- producer ------------------------------------------------------------------------------------------------------------------

// semantics = sum_s w_s logit_s with w_s = (1 - exp(-delta_s sigma_s)) T_s, T_s = exp(-sum_{j<s} delta_j sigma_j), and
//   d semantics / d sigma_s = delta_s [ (T_s - w_s) logit_s - sum_{j>s} w_j logit_j ],   T_s - w_s = T_{s+1}.
// One wavefront per ray, 64 samples per pass in lane order with the running sums carried from chunk to chunk; the first sweep
// gives the ray's total, the second the suffix sums as total - inclusive prefix.
__global__ void __launch_bounds__(256)
semantics_density_gradient_kernel(const float* __restrict__ starts, const float* __restrict__ ends,
                                  const float* __restrict__ density, const float* __restrict__ sem, long long num_rays, int S,
                                  float* __restrict__ out_sem, float* __restrict__ out_w, float* __restrict__ d_density) {
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
  for (long long r = blockIdx.x * (long long)(blockDim.x >> 6) + wave; r < num_rays; r += waves) {
    const long long base = r * (long long)S;
    float total = 0.f;
    for (int sweep = 0; sweep < 2; ++sweep) {
      float carry_dd = 0.f, carry_wl = 0.f, part = 0.f;
      for (int c0 = 0; c0 < S; c0 += 64) {
        const int i = c0 + lane;
        const bool valid = i < S;
        const int ic = valid ? i : S - 1;
        const float delta = ends[base + ic] - starts[base + ic];
        const float logit = valid ? sem[base + ic] : 0.f;
        const float dd = valid ? delta * density[base + ic] : 0.f;
        const float incl = wave_inclusive_scan(dd);
        const float trans = expf(-(carry_dd + (incl - dd)));
        const float w = valid ? nan_to_num((1.f - expf(-dd)) * trans) : 0.f;
        const float wl = valid ? w * logit : 0.f;
        if (sweep == 0) {
          part += wl;
          if (out_w && valid) out_w[base + i] = w;
        } else {
          const float prefix = carry_wl + wave_inclusive_scan(wl);  // sum_{j<=s} w_j logit_j
          const float t_next = expf(-(carry_dd + incl));            // T_{s+1}
          if (valid) d_density[base + i] = delta * (t_next * logit - (total - prefix));
          carry_wl = wave_read(prefix, 63);
        }
        carry_dd += wave_read(incl, 63);
      }
      if (sweep == 0) {
        total = wave_sum(part);
        if (lane == 0) out_sem[r] = total;
      }
    }
  }
}

// d_positions = d_density * d sigma / d x for sigma = exp(h_0) * selector, h = W1 relu(W0 enc(x) + b0) + b1: one thread per sample.
// The gather keeps each level's Jacobian (hash_level_jac: six numbers per level, no second gather); the hidden units are visited
// once -- unit k's pre-activation from row k of W0, and with its gate the same row added to d h_0 / d enc, so a weight is
// loaded once (scalar, the row index is wave-uniform) for two multiply-adds.  Everything lives in registers: 32 encoded values,
// 96 Jacobian entries, 32 gradient sums.  fp32 throughout.  Built for grids of CN_MAX_LEVELS levels (every method of the
// reference): the level loops are unrolled over the register arrays.
struct DensityGradArgs {
  GridDev grid;
  SceneDev scene;
  const float *w0, *b0, *w1, *b1;  // base MLP: [H, 32], [H], row 0 of [1 + geo, H], its bias
  int H;
  const float *origins, *directions, *starts, *ends, *d_density;
  long long total;
  int S;
  float *d_pos, *density;
};

// keeps a level's eight blended values where the program computed them: without it hipcc issues all 128 gathers first and holds
// their 256 raw values (588 bytes of scratch per lane)
__device__ __forceinline__ void pin_level(float2& f, v2f_t& jx, v2f_t& jy, v2f_t& jz) {
  float a = jx.x, b = jx.y, c = jy.x, d = jy.y, e = jz.x, g = jz.y;
  asm volatile("" : "+v"(f.x), "+v"(f.y), "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(g));
  jx = v2f_t{a, b};
  jy = v2f_t{c, d};
  jz = v2f_t{e, g};
}

template <bool HALF>
__global__ void __launch_bounds__(256) field_density_position_gradient_kernel(DensityGradArgs A) {
  constexpr int NL = CN_MAX_LEVELS, IN = 2 * NL;
  const cfloat_ptr W0 = as_const(A.w0), B0 = as_const(A.b0), W1 = as_const(A.w1);
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < A.total; i += stride) {
    const long long r = i / A.S;
    const float mid = (A.starts[i] + A.ends[i]) / 2.f;
    const float wx = A.origins[3 * r] + A.directions[3 * r] * mid;
    const float wy = A.origins[3 * r + 1] + A.directions[3 * r + 1] * mid;
    const float wz = A.origins[3 * r + 2] + A.directions[3 * r + 2] * mid;
    float px = wx, py = wy, pz = wz;
    const bool sel = normalize_position(A.scene, px, py, pz);
    float enc[IN];
    v2f_t jx[NL], jy[NL], jz[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      float2 f = hash_level_jac<HALF>(A.grid.table, A.grid.level(l), A.grid.pos_offset, px, py, pz, jx[l], jy[l], jz[l]);
      pin_level(f, jx[l], jy[l], jz[l]);
      enc[2 * l] = f.x;
      enc[2 * l + 1] = f.y;
    }
    float genc[IN];  // d h_0 / d enc
#pragma unroll
    for (int j = 0; j < IN; ++j) genc[j] = 0.f;
    float logit = A.b1[0];
    for (int k = 0; k < A.H; ++k) {
      float acc = B0[k];
#pragma unroll
      for (int j = 0; j < IN; ++j) acc = fmaf(W0[k * IN + j], enc[j], acc);
      const float c = acc > 0.f ? W1[k] : 0.f;  // ReLU gate times the output row
      logit = fmaf(c, acc, logit);
#pragma unroll
      for (int j = 0; j < IN; ++j) genc[j] = fmaf(W0[k * IN + j], c, genc[j]);
    }
    float gx = 0.f, gy = 0.f, gz = 0.f;  // d h_0 / d (normalised position)
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      gx += genc[2 * l] * jx[l].x + genc[2 * l + 1] * jx[l].y;
      gy += genc[2 * l] * jy[l].x + genc[2 * l + 1] * jy[l].y;
      gz += genc[2 * l] * jz[l].x + genc[2 * l + 1] * jz[l].y;
    }
    // trunc_exp: forward exp(h_0), backward exp(clamp(h_0, -15, 15)); the selector zeroes both
    const float self = sel ? 1.f : 0.f;
    const float dl = A.d_density[i] * self * expf(fminf(fmaxf(logit, -15.f), 15.f));
    gx *= dl;
    gy *= dl;
    gz *= dl;
    normalize_position_backward(A.scene, wx, wy, wz, self, gx, gy, gz);
    A.d_pos[3 * i] = gx;
    A.d_pos[3 * i + 1] = gy;
    A.d_pos[3 * i + 2] = gz;
    if (A.density) A.density[i] = expf(logit) * self;
  }
}

// H[v] += channel_scale * |a_v|^2 with a_v = sum over the (sample, corner) pairs of ONE ray whose literal index is v of
// coef * g (uncertainty.py:60-85: the Jacobian rows of a ray are summed per vertex before the square).  One wavefront per ray
// and one open-addressing table per wavefront in LDS: `slots` (a power of two >= 8 S, so it cannot fill up) records of
// {index, a_x, a_y, a_z}; a lane claims a slot with a compare-and-swap on the index and adds with LDS float atomics, then the
// wave sweeps its table, issues one global float atomic per vertex it met and leaves the table empty for its next ray.
// Deselected samples have coefficient 0 (zero_out=True) and are skipped: they would add 0 to vertex 0.
constexpr unsigned HESS_EMPTY = 0xffffffffu;
__global__ void __launch_bounds__(256)
hessian_accumulate_kernel(const float* __restrict__ origins, const float* __restrict__ directions,
                          const float* __restrict__ starts, const float* __restrict__ ends, const float* __restrict__ d_pos,
                          long long num_rays, int S, SceneDev sc, unsigned L, float channel_scale, unsigned slots,
                          float* __restrict__ hessian) {
  extern __shared__ __align__(16) unsigned hess_lds[];
  const int wave = threadIdx.x >> 6, lane = lane_id(), waves = blockDim.x >> 6;
  unsigned* keys = hess_lds + (size_t)wave * slots * 4u;
  float* acc = reinterpret_cast<float*>(keys + slots);  // [3][slots]
  for (unsigned s = lane; s < slots; s += 64) {
    keys[s] = HESS_EMPTY;
    acc[s] = acc[slots + s] = acc[2 * slots + s] = 0.f;
  }
  __syncthreads();
  const unsigned mask = slots - 1u;
  // every wave of a workgroup makes the same number of trips, so the barriers below are met by all of them
  for (long long r0 = blockIdx.x * (long long)waves; r0 < num_rays; r0 += (long long)gridDim.x * waves) {
    const long long r = r0 + wave;
    if (r < num_rays) {
      const float ox = origins[3 * r], oy = origins[3 * r + 1], oz = origins[3 * r + 2];
      const float dx = directions[3 * r], dy = directions[3 * r + 1], dz = directions[3 * r + 2];
      for (int i = lane; i < S; i += 64) {
        const long long n = r * (long long)S + i;
        const float mid = (starts[n] + ends[n]) / 2.f;
        float px = ox + dx * mid, py = oy + dy * mid, pz = oz + dz * mid;
        if (!normalize_position(sc, px, py, pz)) continue;
        const float gx = d_pos[3 * n], gy = d_pos[3 * n + 1], gz = d_pos[3 * n + 2];
        const GridCorners g = grid_corners(px, py, pz, L);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const unsigned v = g.index(k, L);
          const float c = g.coef(k);
          unsigned s = (v * CN_P1 >> 8) & mask;
          for (;;) {
            const unsigned seen = atomicCAS(&keys[s], HESS_EMPTY, v);
            if (seen == HESS_EMPTY || seen == v) break;
            s = (s + 1u) & mask;
          }
          atomicAdd(&acc[s], c * gx);
          atomicAdd(&acc[slots + s], c * gy);
          atomicAdd(&acc[2 * slots + s], c * gz);
        }
      }
    }
    __syncthreads();
    for (unsigned s = lane; s < slots; s += 64) {
      const unsigned v = keys[s];
      if (v != HESS_EMPTY) {
        const float ax = acc[s], ay = acc[slots + s], az = acc[2 * slots + s];
        const float h = channel_scale * (ax * ax + ay * ay + az * az);
        if (h != 0.f) atomicAdd(hessian + v, h);
        keys[s] = HESS_EMPTY;
        acc[s] = acc[slots + s] = acc[2 * slots + s] = 0.f;
      }
    }
    __syncthreads();
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

extern "C" int cn_semantics_density_gradient(const float* starts, const float* ends, const float* density,
                                             const float* semantics, int64_t num_rays, int32_t num_samples,
                                             float* rendered_semantics, float* weights, float* d_density, cn_stream_t stream) {
  CN_REQUIRE(starts && ends && density && semantics && rendered_semantics && d_density, CN_ERR_INVALID,
             "cn_semantics_density_gradient: null starts/ends/density/semantics/rendered_semantics/d_density");
  CN_REQUIRE(num_samples > 0, CN_ERR_INVALID, "cn_semantics_density_gradient: num_samples must be > 0");
  if (num_rays <= 0) return CN_OK;
  hipLaunchKernelGGL(cn::semantics_density_gradient_kernel, dim3(cn::grid_for(num_rays, 4, 16384)), dim3(256), 0,
                     cn::as_stream(stream), starts, ends, density, semantics, (long long)num_rays, num_samples,
                     rendered_semantics, weights, d_density);
  return cn::check_launch("cn_semantics_density_gradient");
}

extern "C" int cn_field_density_position_gradient(const cn_field_params* params, const cn_scene* scene, const float* origins,
                                                  const float* directions, const float* starts, const float* ends,
                                                  const float* d_density, int64_t num_rays, int32_t num_samples,
                                                  float* d_positions, float* density, cn_stream_t stream) {
  const char* who = "cn_field_density_position_gradient";
  CN_REQUIRE(params && scene && origins && directions && starts && ends && d_density && d_positions, CN_ERR_INVALID,
             "%s: null params/scene/origins/directions/starts/ends/d_density/d_positions", who);
  CN_REQUIRE(num_samples > 0, CN_ERR_INVALID, "%s: num_samples must be > 0", who);
  if (int rc = cn::check_grid(params->grid, false, who)) return rc;
  const cn_mlp& b = params->base;
  CN_REQUIRE(params->grid.num_levels == CN_MAX_LEVELS, CN_ERR_UNSUPPORTED, "%s: %d grid levels (built for %d)", who,
             params->grid.num_levels, CN_MAX_LEVELS);
  CN_REQUIRE(b.num_layers == 2 && b.dims[0] == 2 * CN_MAX_LEVELS && b.dims[1] >= 1 && b.dims[1] <= 128 && b.dims[2] >= 1,
             CN_ERR_UNSUPPORTED, "%s: base MLP of %d layers, %d -> %d -> %d (built for 2 layers, 32 inputs, width <= 128)", who,
             b.num_layers, b.dims[0], b.dims[1], b.dims[2]);
  CN_REQUIRE(b.weight[0] && b.bias[0] && b.weight[1] && b.bias[1], CN_ERR_INVALID, "%s: null base MLP weights", who);
  if (num_rays <= 0) return CN_OK;
  cn::DensityGradArgs A;
  A.grid = cn::make_grid_dev(params->grid);
  A.scene = cn::make_scene_dev(*scene);
  A.w0 = b.weight[0];
  A.b0 = b.bias[0];
  A.w1 = b.weight[1];  // row 0 of [1 + geo, H]: the density logit
  A.b1 = b.bias[1];
  A.H = b.dims[1];
  A.origins = origins;
  A.directions = directions;
  A.starts = starts;
  A.ends = ends;
  A.d_density = d_density;
  A.total = (long long)num_rays * num_samples;
  A.S = num_samples;
  A.d_pos = d_positions;
  A.density = density;
  const dim3 grid(cn::grid_for(A.total, 256, 1 << 20)), block(256);
  hipStream_t st = cn::as_stream(stream);
  if (A.grid.half) hipLaunchKernelGGL(cn::field_density_position_gradient_kernel<true>, grid, block, 0, st, A);
  else hipLaunchKernelGGL(cn::field_density_position_gradient_kernel<false>, grid, block, 0, st, A);
  return cn::check_launch(who);
}

extern "C" int cn_hessian_accumulate(const float* origins, const float* directions, const float* starts, const float* ends,
                                     const float* d_positions, int64_t num_rays, int32_t num_samples, const cn_scene* scene,
                                     int32_t lod, float channel_scale, float* hessian, cn_stream_t stream) {
  CN_REQUIRE(origins && directions && starts && ends && d_positions && scene && hessian, CN_ERR_INVALID,
             "cn_hessian_accumulate: null origins/directions/starts/ends/d_positions/scene/hessian");
  CN_REQUIRE(num_samples > 0, CN_ERR_INVALID, "cn_hessian_accumulate: num_samples must be > 0");
  CN_REQUIRE(num_samples <= 256, CN_ERR_UNSUPPORTED, "cn_hessian_accumulate: %d samples per ray (built for <= 256)", num_samples);
  if (int rc = check_lod(lod, "cn_hessian_accumulate")) return rc;
  const unsigned long long L = 1ull << lod;
  // the bound cn_uncertainty_lookup checks: the largest literal index is L^3 + L^2 + L
  CN_REQUIRE(L * L * L + L * L + L < (L + 1) * (L + 1) * (L + 1), CN_ERR_INVALID,
             "cn_hessian_accumulate: corner indices leave the table at lod %d", lod);
  if (num_rays <= 0) return CN_OK;
  // a ray meets at most 8 S vertices; twice that many slots (a power of two) up to the 64 KiB a workgroup may hold, where one
  // wave with S > 128 still gets 4096 >= 8 S
  unsigned slots = 64;
  while (slots < 16u * (unsigned)num_samples && slots < 4096u) slots <<= 1;
  int waves = (int)(65536u / (slots * 16u));
  if (waves > 4) waves = 4;
  hipLaunchKernelGGL(cn::hessian_accumulate_kernel, dim3(cn::grid_for(num_rays, waves, 16384)), dim3(64 * waves),
                     (size_t)waves * slots * 16u, cn::as_stream(stream), origins, directions, starts, ends, d_positions,
                     (long long)num_rays, num_samples, cn::make_scene_dev(*scene), (unsigned)L, channel_scale, slots, hessian);
  return cn::check_launch("cn_hessian_accumulate");
}
