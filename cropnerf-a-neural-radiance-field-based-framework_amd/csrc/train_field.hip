// Training, field side: parameter gradients of FruitField and of the proposal HashMLPDensityFields.  Given
// d loss / d (density, rgb, semantics) per sample (train_render.hip) -- d loss / d density for a proposal network (interlevel
// loss) -- an entry recomputes the network's forward tile by tile with the activations in LDS, back-propagates, and
// accumulates the gradients of every Linear layer, of the appearance embedding and of the hash table.
//
// This file is the unit's HOST code: argument checks, the scatter plan, launches.  Every kernel is in a header:
//
//   entry (and its _mp / _ex spellings)   kernel launched by default                    older form, and its switch
//   cn_field_backward                     mf::field_backward_mfma_kernel                field_backward_kernel (scalar FMAs),
//     default fruit_nerf_method shape       train_field_mfma.hpp                          train_field_scalar.hpp,
//     (16 levels, 32->64->16,                                                             CN_FIELD_BACKWARD_IMPL=scalar
//     15->64->64->1, 63->64->64->3, app 32)
//   cn_field_backward_general             gb::field_backward_general_kernel, then       --
//     _big / _huge and every other shape    gb::field_backward_reduce_all_kernel,
//     of the family general_family_ok       train_field_general.hpp
//   cn_proposal_backward                  pw::proposal_backward_wave_kernel             proposal_backward_kernel (four waves per
//     {5|7}-level 2L->16->1 nets            train_proposal_wave.hpp                       tile), train_proposal_tile.hpp,
//                                                                                         CN_PROP_BWD=tile
//
// Other shapes return CN_ERR_UNSUPPORTED.  The older forms stay as independent device implementations that tests compare
// the defaults against.  Hash-table gradients are scatter-adds (2 floats x 8 corners per level per sample); how they reach
// the table -- directly, through private copies of level 0, or through cell-major records (CN_CELL_SCATTER=<cells per
// sample>, 0: off) -- the fold kernels, and the plan / finish pair the entries bracket their kernel with are
// grid_scatter.hpp.  train_field_common.hpp holds the kernel argument structs.  All of it is one translation unit: the
// headers define __global__ functions.
// The fullest spelling of a field family (cn_field_backward_ex, cn_field_backward_general_mp) holds the body; the shorter
// ones call it directly.
#include <algorithm>
#include <cstring>
#include <cstdlib>

#include "grid_scatter.hpp"
#include "train_field_general.hpp"
#include "train_field_mfma.hpp"
#include "train_field_scalar.hpp"
#include "train_proposal_tile.hpp"
#include "train_proposal_wave.hpp"

namespace cn {

int validate_field(const cn_field_params& p);  // field_simple.hip

static bool is_default_field_shape(const cn_field_params& p) {
  return p.grid.num_levels == 16 && p.geo_feat_dim == 15 && p.app_dim == 32 && p.base.num_layers == 2 &&
         p.base.dims[0] == 32 && p.base.dims[1] == 64 && p.base.dims[2] == 16 && p.semantics.num_layers == 2 &&
         p.semantics.dims[0] == 15 && p.semantics.dims[1] == 64 && p.semantics.dims[2] == 64 &&
         p.color.num_layers == 3 && p.color.dims[0] == 63 && p.color.dims[1] == 64 && p.color.dims[2] == 64 &&
         p.color.dims[3] == 3;
}

// The checks cn_field_backward and cn_field_backward_general share, under the entry's name (the two families word the
// app_mean message differently: `app_mean_tail`).  `shape_ok` runs on validated parameters.
static int check_field_backward_args(const char* entry, const char* app_mean_tail,
                                     bool (*shape_ok)(const cn_field_params&, const cn_field_params&), const char* shape_msg,
                                     const cn_field_params* params, const cn_field_params* grads, const cn_scene* scene,
                                     int32_t app_mode, const float* app_mean, const float* origins, const float* directions,
                                     const int64_t* camera_indices, const float* starts, const float* ends,
                                     const float* d_density, const float* d_rgb, const float* d_semantics,
                                     int32_t matrix_precision, uint32_t flags) {
  CN_REQUIRE(params && grads && scene && origins && directions && starts && ends && d_density && d_rgb && d_semantics,
             CN_ERR_INVALID, "%s: null argument", entry);
  CN_REQUIRE(matrix_precision == CN_MATRIX_FP32 || matrix_precision == CN_MATRIX_SPLIT_BF16 || matrix_precision == CN_MATRIX_F16,
             CN_ERR_INVALID, "%s: matrix_precision %d", entry, matrix_precision);
  CN_REQUIRE((flags & ~TRAIN_FLAGS_ALL) == 0, CN_ERR_INVALID, "%s: unknown flags 0x%x", entry, (unsigned)flags);
  // (CN_TRAIN_GRADIENT_SCALING needs nothing here: the render backward hands over scaled per-sample gradients)
  CN_REQUIRE(app_mode != CN_APP_PER_CAMERA || camera_indices, CN_ERR_INVALID, "Camera indices are not provided.");
  CN_REQUIRE(app_mode != CN_APP_MEAN || app_mean, CN_ERR_INVALID, "%s: app_mean required%s", entry, app_mean_tail);
  int rc = validate_field(*params);
  if (rc) return rc;
  if ((rc = validate_field(*grads))) return rc;
  CN_REQUIRE(shape_ok(*params, *grads), CN_ERR_UNSUPPORTED, "%s", shape_msg);
  return check_grad_grid(params->grid, grads->grid, entry);
}

// ---- shape-generic field backward ------------------------------------------------------------------------------------------
static bool general_family_ok(const cn_field_params& p) {
  auto w128 = [](const cn_mlp& m) {
    for (int l = 0; l <= m.num_layers; ++l)
      if (m.dims[l] > 128) return false;
    return true;
  };
  return p.base.num_layers == 2 && (p.semantics.num_layers == 2 || p.semantics.num_layers == 3) &&
         p.color.num_layers == 3 && w128(p.base) && w128(p.semantics) && w128(p.color) && p.geo_feat_dim <= 30 &&
         2 * p.grid.num_levels <= 32 && 16 + p.geo_feat_dim + p.app_dim <= 128;
}
// floats of one workgroup's scratch slice: every parameter tensor starts on a 64-byte line (a 16-float segment of a weight
// row that straddles two lines costs two L2 requests each way: 5 240 write requests per tile instead of 3 212, measured)
static int general_pad16(int n) { return (n + 15) & ~15; }
static int general_param_count(const cn_field_params& p) {
  auto mlp = [](const cn_mlp& m) {
    int n = 0;
    for (int l = 0; l < m.num_layers; ++l) n += general_pad16(m.dims[l] * m.dims[l + 1]) + general_pad16(m.dims[l + 1]);
    return n;
  };
  return mlp(p.base) + mlp(p.semantics) + mlp(p.color) + general_pad16(p.semantics.dims[p.semantics.num_layers]) + 16;
}
static int general_blocks() {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  return cus;
}
// the same, rounded up to whole float4s: the slice of the caller's workspace one workgroup owns
static int general_params_per_block(const cn_field_params& p) { return (general_param_count(p) + 3) / 4 * 4; }

}  // namespace cn

// ---- the exported entries: the fullest spelling of a family holds the body, the shorter ones call it directly -------------
extern "C" int cn_field_backward(const cn_field_params* params, const cn_field_params* grads, const cn_scene* scene,
                                 int32_t app_mode, int32_t sh_unit_dir, const float* app_mean, const float* origins,
                                 const float* directions, const int64_t* camera_indices, const float* starts,
                                 const float* ends, const float* d_density, const float* d_rgb, const float* d_semantics,
                                 int64_t num_rays, int32_t num_samples, float* d_positions, float* d_directions,
                                 cn_stream_t stream) {
  return cn_field_backward_ex(params, grads, scene, app_mode, sh_unit_dir, app_mean, origins, directions, camera_indices, starts,
                              ends, d_density, d_rgb, d_semantics, num_rays, num_samples, d_positions, d_directions,
                              CN_MATRIX_FP32, 0u, stream);
}

extern "C" int cn_field_backward_mp(const cn_field_params* params, const cn_field_params* grads, const cn_scene* scene,
                                    int32_t app_mode, int32_t sh_unit_dir, const float* app_mean, const float* origins,
                                    const float* directions, const int64_t* camera_indices, const float* starts,
                                    const float* ends, const float* d_density, const float* d_rgb, const float* d_semantics,
                                    int64_t num_rays, int32_t num_samples, float* d_positions, float* d_directions,
                                    int32_t matrix_precision, cn_stream_t stream) {
  return cn_field_backward_ex(params, grads, scene, app_mode, sh_unit_dir, app_mean, origins, directions, camera_indices, starts,
                              ends, d_density, d_rgb, d_semantics, num_rays, num_samples, d_positions, d_directions,
                              matrix_precision, 0u, stream);
}

extern "C" int cn_field_backward_ex(const cn_field_params* params, const cn_field_params* grads, const cn_scene* scene,
                                    int32_t app_mode, int32_t sh_unit_dir, const float* app_mean, const float* origins,
                                    const float* directions, const int64_t* camera_indices, const float* starts,
                                    const float* ends, const float* d_density, const float* d_rgb, const float* d_semantics,
                                    int64_t num_rays, int32_t num_samples, float* d_positions, float* d_directions,
                                    int32_t matrix_precision, uint32_t flags, cn_stream_t stream) {
  int rc = cn::check_field_backward_args(
      "cn_field_backward", " for CN_APP_MEAN",
      [](const cn_field_params& p, const cn_field_params& g) {
        return cn::is_default_field_shape(p) && cn::is_default_field_shape(g);
      },
      "cn_field_backward is built for the default fruit_nerf_method field shape", params, grads, scene, app_mode, app_mean,
      origins, directions, camera_indices, starts, ends, d_density, d_rgb, d_semantics, matrix_precision, flags);
  if (rc) return rc;
  const bool pass_sem = (flags & CN_TRAIN_PASS_SEMANTIC_GRADIENTS) != 0;
  if (num_rays <= 0) return CN_OK;
  cn::FieldBwdArgs A{};
  auto fill = [](auto& dst, const cn_field_params& s) {
    dst.w0 = (decltype(dst.w0))s.base.weight[0];
    dst.b0 = (decltype(dst.b0))s.base.bias[0];
    dst.w1 = (decltype(dst.w1))s.base.weight[1];
    dst.b1 = (decltype(dst.b1))s.base.bias[1];
    dst.ws0 = (decltype(dst.ws0))s.semantics.weight[0];
    dst.bs0 = (decltype(dst.bs0))s.semantics.bias[0];
    dst.ws1 = (decltype(dst.ws1))s.semantics.weight[1];
    dst.bs1 = (decltype(dst.bs1))s.semantics.bias[1];
    dst.wh = (decltype(dst.wh))s.sem_head_weight;
    dst.bh = (decltype(dst.bh))s.sem_head_bias;
    dst.wc0 = (decltype(dst.wc0))s.color.weight[0];
    dst.bc0 = (decltype(dst.bc0))s.color.bias[0];
    dst.wc1 = (decltype(dst.wc1))s.color.weight[1];
    dst.bc1 = (decltype(dst.bc1))s.color.bias[1];
    dst.wc2 = (decltype(dst.wc2))s.color.weight[2];
    dst.bc2 = (decltype(dst.bc2))s.color.bias[2];
    dst.emb = (decltype(dst.emb))s.appearance;
    dst.table = (decltype(dst.table))s.grid.table;
  };
  fill(A.p, *params);
  fill(A.g, *grads);
  A.grid = cn::make_grid_dev(params->grid);
  A.scene = cn::make_scene_dev(*scene);
  A.sh_unit = sh_unit_dir;
  A.app_per_camera = app_mode == CN_APP_PER_CAMERA;
  A.app_mean = app_mode == CN_APP_MEAN ? app_mean : nullptr;
  A.origins = origins;
  A.directions = directions;
  A.starts = starts;
  A.ends = ends;
  A.cam_idx = camera_indices;
  A.d_density = d_density;
  A.d_rgb = d_rgb;
  A.d_sem = d_semantics;
  A.d_pos = d_positions;
  A.d_dir = d_directions;
  A.R = num_rays;
  A.S = num_samples;
  // default: the matrix-core kernel; CN_FIELD_BACKWARD_IMPL=scalar selects the first (scalar-FMA) implementation,
  // kept as an independent device implementation for cross-checks
  const char* impl_env = getenv("CN_FIELD_BACKWARD_IMPL");  // read per call: one process can compare both
  const bool use_scalar = impl_env && std::strcmp(impl_env, "scalar") == 0;
  CN_REQUIRE(!(use_scalar && pass_sem), CN_ERR_UNSUPPORTED,
             "cn_field_backward: the scalar implementation (CN_FIELD_BACKWARD_IMPL=scalar) runs the semantic branch after the "
             "base-MLP backward and does not implement CN_TRAIN_PASS_SEMANTIC_GRADIENTS");
  // [f16][pass_sem]  (split-bf16 keeps ~fp32 products in the forward; its gradient is the exact-fp32 kernel's)
  using cn::mf::field_backward_mfma_kernel;
  typedef void (*MfmaKernel)(cn::FieldBwdArgs);
  static const MfmaKernel mfma_kernels[2][2] = {{field_backward_mfma_kernel<0>, field_backward_mfma_kernel<0, true>},
                                                {field_backward_mfma_kernel<1>, field_backward_mfma_kernel<1, true>}};
  static cn::PerDevice<int> attrs;  // one-time kernel attributes, per device
  rc = attrs.get(
      [](int, int&) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cn::field_backward_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)((size_t)cn::FIELD_ROWS * cn::LD * sizeof(float)));
        if (e != hipSuccess) return e;
        for (const auto& row : mfma_kernels)
          for (const MfmaKernel k : row) {
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)cn::mf::LDS_BYTES);
            if (e != hipSuccess) return e;
          }
        return hipSuccess;
      },
      nullptr, "cn_field_backward");
  if (rc) return rc;
  const long long nsamp = num_rays * (long long)num_samples;
  if (use_scalar) {  // every level on the table path: no scatter plan, nothing to fold
    size_t lds = (size_t)cn::FIELD_ROWS * cn::LD * sizeof(float);
    long long ntiles = (nsamp + cn::TS - 1) / cn::TS;
    hipLaunchKernelGGL(cn::field_backward_kernel, dim3(cn::grid_for(ntiles, 1, 256)), dim3(cn::TB), lds,
                       cn::as_stream(stream), A);
    if ((rc = cn::check_launch("cn_field_backward"))) return rc;
    CN_DET_FLUSH(cn::as_stream(stream));
    return CN_OK;
  }
  long long ntiles = (nsamp + cn::mf::TSM - 1) / cn::mf::TSM;
  // cell-major records for the levels with at most CELL_RATIO_FIELD cells per sample (CN_CELL_SCATTER=<ratio>, 0: off)
  cn::plan_grid_scatter(grads->grid, (unsigned long long)nsamp, cn::CELL_RATIO_FIELD, true, A.coarse, A.cells);
  hipLaunchKernelGGL(mfma_kernels[matrix_precision == CN_MATRIX_F16][pass_sem], dim3(cn::grid_for(ntiles, 1, 256)),
                     dim3(cn::mf::NT), cn::mf::LDS_BYTES, cn::as_stream(stream), A);
  return cn::finish_grid_scatter(A.coarse, A.cells, A.grid, A.g.table, cn::as_stream(stream), "cn_field_backward");
}

extern "C" int cn_proposal_backward(const cn_density_params* params, const cn_density_params* grads,
                                    const cn_scene* scene, const float* origins, const float* directions,
                                    const float* starts, const float* ends, const float* d_density, int64_t num_rays,
                                    int32_t num_samples, float* d_positions, cn_stream_t stream) {
  CN_REQUIRE(params && grads && scene && origins && directions && starts && ends && d_density, CN_ERR_INVALID,
             "cn_proposal_backward: null argument");
  int rc = cn::check_grad_grid(params->grid, grads->grid, "cn_proposal_backward");
  if (rc) return rc;
  const int L = params->grid.num_levels;
  bool ok = (L == 5 || L == 7) && params->mlp.num_layers == 2 && params->mlp.dims[0] == 2 * L &&
            params->mlp.dims[1] == 16 && params->mlp.dims[2] == 1 && grads->grid.num_levels == L &&
            grads->grid.log2_table_size == params->grid.log2_table_size;
  CN_REQUIRE(ok, CN_ERR_UNSUPPORTED, "cn_proposal_backward: proposal net must be {5|7 levels, 2L->16->1}");
  CN_REQUIRE(grads->grid.table && grads->mlp.weight[0] && grads->mlp.bias[0] && grads->mlp.weight[1] &&
                 grads->mlp.bias[1],
             CN_ERR_INVALID, "cn_proposal_backward: null gradient buffer");
  if (num_rays <= 0) return CN_OK;
  cn::PropBwdArgs A{};
  A.table = static_cast<const float*>(params->grid.table);
  A.w0 = params->mlp.weight[0];
  A.b0 = params->mlp.bias[0];
  A.w1 = params->mlp.weight[1];
  A.b1 = params->mlp.bias[1];
  A.g_table = static_cast<float*>(const_cast<void*>(grads->grid.table));
  A.g_w0 = const_cast<float*>(grads->mlp.weight[0]);
  A.g_b0 = const_cast<float*>(grads->mlp.bias[0]);
  A.g_w1 = const_cast<float*>(grads->mlp.weight[1]);
  A.g_b1 = const_cast<float*>(grads->mlp.bias[1]);
  A.grid = cn::make_grid_dev(params->grid);
  A.scene = cn::make_scene_dev(*scene);
  A.origins = origins;
  A.directions = directions;
  A.starts = starts;
  A.ends = ends;
  A.d_density = d_density;
  A.d_pos = d_positions;
  A.R = num_rays;
  A.S = num_samples;
  // cell-major records for the levels with at most CELL_RATIO_PROPOSAL cells per sample (runs of a ray's samples merge there);
  // CN_CELL_SCATTER = 0 keeps every level on the table path
  cn::plan_grid_scatter(grads->grid, (unsigned long long)num_rays * (unsigned long long)num_samples, cn::CELL_RATIO_PROPOSAL,
                        true, A.coarse, A.cells);
  long long ntiles = (num_rays * (long long)num_samples + cn::TS - 1) / cn::TS;
  // one wave per tile (train_proposal_wave.hpp); CN_PROP_BWD=tile: the first form, four waves per tile (A/B runs, cross-check)
  const char* form = getenv("CN_PROP_BWD");
  const bool tile = form && strcmp(form, "tile") == 0;
  typedef void (*PropKernel)(cn::PropBwdArgs);
  const PropKernel kernel =
      tile ? (L == 5 ? cn::proposal_backward_kernel<5> : cn::proposal_backward_kernel<7>)
           : (L == 5 ? cn::pw::proposal_backward_wave_kernel<5> : cn::pw::proposal_backward_wave_kernel<7>);
  hipLaunchKernelGGL(kernel, dim3(cn::grid_for(tile ? ntiles : (ntiles + 3) / 4, 1, 1024)), dim3(cn::TB), 0,
                     cn::as_stream(stream), A);
  return cn::finish_grid_scatter(A.coarse, A.cells, A.grid, A.g_table, cn::as_stream(stream), "cn_proposal_backward");
}

extern "C" size_t cn_grid_scatter_scratch_bytes(const cn_grid* grid) {
  if (!grid || grid->num_levels < 1) return 0;
  const size_t head = cn::coarse_scratch_bytes(*grid);
  return head ? head + cn::cell_scratch_layout(*grid, nullptr) : 0;
}

// The same, sized for batches of at most `max_samples` samples per backward call: a level is kept cell-major only when it
// has at most (CN_CELL_SCATTER; defaults CELL_RATIO_FIELD / CELL_RATIO_PROPOSAL, at most
// CELL_RATIO_MAX) x samples cells, so the records of levels with more than CELL_RATIO_MAX x max_samples cells would never be
// touched.  max_samples <= 0: every level up to CELL_MAX_CELLS cells (= cn_grid_scatter_scratch_bytes).
extern "C" size_t cn_grid_scatter_scratch_bytes_for(const cn_grid* grid, int64_t max_samples) {
  if (!grid || grid->num_levels < 1) return 0;
  const size_t head = cn::coarse_scratch_bytes(*grid);
  if (!head) return 0;
  cn::CellScatter c{};
  const size_t all = cn::cell_scratch_layout(*grid, &c);
  if (max_samples <= 0) return head + all;
  size_t bytes = 0;
  for (int l = 0; l < c.num_levels; ++l) {
    const unsigned long long cells = (unsigned long long)c.n[l] * c.n[l] * c.n[l];
    if ((double)cells > cn::CELL_RATIO_MAX * (double)max_samples) break;
    bytes = (size_t)(c.offset[l] + c.copies[l] * cells * 16ull) * sizeof(float);
  }
  return head + bytes;
}

extern "C" size_t cn_field_backward_general_workspace_bytes(const cn_field_params* params) {
  if (!params) return 0;
  return (size_t)cn::general_blocks() * cn::general_params_per_block(*params) * sizeof(float);
}

extern "C" int cn_field_backward_general(const cn_field_params* params, const cn_field_params* grads, const cn_scene* scene,
                                         int32_t app_mode, int32_t sh_unit_dir, const float* app_mean, const float* origins,
                                         const float* directions, const int64_t* camera_indices, const float* starts,
                                         const float* ends, const float* d_density, const float* d_rgb, const float* d_semantics,
                                         int64_t num_rays, int32_t num_samples, float* d_positions, float* d_directions,
                                         void* workspace, size_t workspace_bytes, cn_stream_t stream) {
  return cn_field_backward_general_mp(params, grads, scene, app_mode, sh_unit_dir, app_mean, origins, directions, camera_indices, starts,
                                         ends, d_density, d_rgb, d_semantics, num_rays, num_samples, d_positions, d_directions,
                                         0u, CN_MATRIX_FP32, workspace, workspace_bytes, stream);
}

extern "C" int cn_field_backward_general_ex(const cn_field_params* params, const cn_field_params* grads, const cn_scene* scene,
                                            int32_t app_mode, int32_t sh_unit_dir, const float* app_mean, const float* origins,
                                            const float* directions, const int64_t* camera_indices, const float* starts,
                                            const float* ends, const float* d_density, const float* d_rgb, const float* d_semantics,
                                            int64_t num_rays, int32_t num_samples, float* d_positions, float* d_directions,
                                            uint32_t flags, void* workspace, size_t workspace_bytes, cn_stream_t stream) {
  return cn_field_backward_general_mp(params, grads, scene, app_mode, sh_unit_dir, app_mean, origins, directions, camera_indices, starts,
                                         ends, d_density, d_rgb, d_semantics, num_rays, num_samples, d_positions, d_directions,
                                         flags, CN_MATRIX_FP32, workspace, workspace_bytes, stream);
}

extern "C" int cn_field_backward_general_mp(const cn_field_params* params, const cn_field_params* grads, const cn_scene* scene,
                                            int32_t app_mode, int32_t sh_unit_dir, const float* app_mean, const float* origins,
                                            const float* directions, const int64_t* camera_indices, const float* starts,
                                            const float* ends, const float* d_density, const float* d_rgb, const float* d_semantics,
                                            int64_t num_rays, int32_t num_samples, float* d_positions, float* d_directions,
                                            uint32_t flags, int32_t matrix_precision, void* workspace, size_t workspace_bytes,
                                            cn_stream_t stream) {
  int rc = cn::check_field_backward_args(
      "cn_field_backward_general", "",
      [](const cn_field_params& p, const cn_field_params&) { return cn::general_family_ok(p); },
      "cn_field_backward_general: base 2 layers, semantics 2-3 layers, colour 3 layers, widths <= 128", params, grads, scene,
      app_mode, app_mean, origins, directions, camera_indices, starts, ends, d_density, d_rgb, d_semantics, matrix_precision,
      flags);
  if (rc) return rc;
  if (num_rays <= 0) return CN_OK;
  const int nblk = cn::general_blocks();
  const int ppb = cn::general_params_per_block(*params);
  CN_REQUIRE(workspace && workspace_bytes >= (size_t)nblk * ppb * sizeof(float), CN_ERR_WORKSPACE,
             "cn_field_backward_general: workspace %zu B < %zu B", workspace_bytes, (size_t)nblk * ppb * sizeof(float));
  hipStream_t s = cn::as_stream(stream);
  cn::gb::GenArgs A{};
  int off = 0;
  struct Target { float* g; int off, n; };
  Target targets[24];
  int nt = 0;
  auto fill = [&](cn::gb::GenLayer* dst, const cn_mlp& m, const cn_mlp& gm) {
    for (int l = 0; l < m.num_layers; ++l) {
      dst[l].W = m.weight[l];
      dst[l].b = m.bias[l];
      dst[l].K = m.dims[l];
      dst[l].N = m.dims[l + 1];
      dst[l].off_w = off;
      targets[nt++] = {const_cast<float*>(gm.weight[l]), off, m.dims[l] * m.dims[l + 1]};
      off += cn::general_pad16(m.dims[l] * m.dims[l + 1]);
      dst[l].off_b = off;
      targets[nt++] = {const_cast<float*>(gm.bias[l]), off, m.dims[l + 1]};
      off += cn::general_pad16(m.dims[l + 1]);
    }
  };
  fill(A.base, params->base, grads->base);
  fill(A.sem, params->semantics, grads->semantics);
  fill(A.col, params->color, grads->color);
  A.ns = params->semantics.num_layers;
  const int ht = params->semantics.dims[A.ns];
  A.wh = params->sem_head_weight;
  A.off_wh = off;
  targets[nt++] = {const_cast<float*>(grads->sem_head_weight), off, ht};
  off += cn::general_pad16(ht);
  A.off_bh = off;
  targets[nt++] = {const_cast<float*>(grads->sem_head_bias), off, 1};
  off += 16;
  CN_REQUIRE(off == cn::general_param_count(*params), CN_ERR_WORKSPACE, "cn_field_backward_general: scratch layout %d != %d", off,
             cn::general_param_count(*params));
  for (int i = 0; i < nt; ++i) CN_REQUIRE(targets[i].g, CN_ERR_INVALID, "cn_field_backward_general: null gradient buffer");
  A.params_per_block = ppb;
  A.scratch = static_cast<float*>(workspace);
  int rows = 0, wmax = 16;
  auto take = [&](int n) { int r = rows; rows += n; return r; };
  const int enc = 2 * params->grid.num_levels, cin = 16 + params->geo_feat_dim + params->app_dim;
  for (const cn_mlp* m : {&params->base, &params->semantics, &params->color})
    for (int l = 0; l <= m->num_layers; ++l) wmax = std::max(wmax, cn::general_pad16(m->dims[l]));
  A.r_enc = take(cn::general_pad16(enc));
  A.r_h1 = take(cn::general_pad16(params->base.dims[1]));
  A.r_g = take(48);
  for (int l = 0; l < A.ns; ++l) A.r_s[l] = take(cn::general_pad16(params->semantics.dims[l + 1]));
  A.r_cin = take(cn::general_pad16(cin));
  A.r_c1 = take(cn::general_pad16(params->color.dims[1]));
  A.r_c2 = take(cn::general_pad16(params->color.dims[2]));
  A.r_rgb = take(16);
  A.r_da = take(std::max(wmax, 48));  // also the 16 x 3 position-gradient partials
  A.r_db = take(wmax);
  A.r_dcin = take(cn::general_pad16(cin));
  A.r_dg = take(32);
  A.r_drgb = take(16);
  A.r_dsem = take(16);
  A.rows = rows;
  const size_t lds = ((size_t)rows * cn::gb::LDG + cn::LVL_REC_FLOATS) * sizeof(float);
  CN_REQUIRE(lds <= 160 * 1024, CN_ERR_UNSUPPORTED,
             "cn_field_backward_general: the activations of one 32-sample tile need %zu B of LDS (max 163840)", lds);
  A.table = static_cast<const float*>(params->grid.table);
  A.g_table = static_cast<float*>(const_cast<void*>(grads->grid.table));
  A.emb = params->appearance;
  A.g_emb = const_cast<float*>(grads->appearance);
  A.app_mean = app_mode == CN_APP_MEAN ? app_mean : nullptr;
  A.grid = cn::make_grid_dev(params->grid);
  A.num_levels = params->grid.num_levels;
  A.geo = params->geo_feat_dim;
  A.app_dim = params->app_dim;
  A.app_per_camera = app_mode == CN_APP_PER_CAMERA;
  A.sh_unit = sh_unit_dir;
  A.scene = cn::make_scene_dev(*scene);
  A.origins = origins;
  A.directions = directions;
  A.starts = starts;
  A.ends = ends;
  A.cam_idx = camera_indices;
  A.d_density = d_density;
  A.d_rgb = d_rgb;
  A.d_sem = d_semantics;
  A.d_pos = d_positions;
  A.d_dir = d_directions;
  A.R = num_rays;
  A.S = num_samples;
  A.pass_sem = (flags & CN_TRAIN_PASS_SEMANTIC_GRADIENTS) ? 1 : 0;
  CN_REQUIRE(A.g_table && (!A.app_per_camera || A.g_emb), CN_ERR_INVALID, "cn_field_backward_general: null gradient buffer");
  // CN_MATRIX_F16: the mixed-precision kernel; CN_MATRIX_SPLIT_BF16 (a ~fp32 forward) trains in exact fp32, as cn_field_backward
  typedef void (*GenKernel)(cn::gb::GenArgs);
  const GenKernel kernel = matrix_precision == CN_MATRIX_F16 ? cn::gb::field_backward_general_kernel<1>
                                                             : cn::gb::field_backward_general_kernel<0>;
  // (the LDS need depends on the field shape, so the attribute is set per call: cheap, and correct on every device)
  CN_REQUIRE(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess,
             CN_ERR_LAUNCH, "cn_field_backward_general: hipFuncSetAttribute(MaxDynamicSharedMemorySize, %zu) failed", lds);
  CN_REQUIRE(hipMemsetAsync(workspace, 0, (size_t)nblk * ppb * sizeof(float), s) == hipSuccess, CN_ERR_LAUNCH,
             "cn_field_backward_general: hipMemsetAsync failed");
  const long long ntiles = (num_rays * (long long)num_samples + cn::gb::TSG - 1) / cn::gb::TSG;
  const int grid = (int)std::min<long long>(ntiles, nblk);
  // cell-major records (as in cn_field_backward) when the four LDS buffers that carry the hand-over hold two waves each
  const int small = std::min(std::min(cn::general_pad16(params->color.dims[1]), cn::general_pad16(params->color.dims[2])),
                             cn::general_pad16(cin));
  cn::plan_grid_scatter(grads->grid, (unsigned long long)num_rays * (unsigned long long)num_samples, cn::CELL_RATIO_FIELD,
                        small * cn::gb::LDG >= 2 * 64 * 17 && A.num_levels <= 16, A.coarse, A.cells,
                        num_rays * (double)num_samples);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(cn::gb::NTG), lds, s, A);
  if ((rc = cn::finish_grid_scatter(A.coarse, A.cells, A.grid, A.g_table, s, "cn_field_backward_general"))) return rc;
  cn::gb::ReduceTargets T;
  T.count = nt;
  for (int i = 0; i < nt; ++i) {
    T.g[i] = targets[i].g;
    T.off[i] = targets[i].off;
    T.n[i] = targets[i].n;
  }
  hipLaunchKernelGGL(cn::gb::field_backward_reduce_all_kernel, dim3((ppb + 31) / 32), dim3(256), 0, s, A.scratch, grid, ppb, T);
  return cn::check_launch("cn_field_backward_general reduce");
}
