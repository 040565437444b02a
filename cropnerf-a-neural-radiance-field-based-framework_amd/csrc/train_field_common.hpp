// What the kernels of the training backward unit (train_field.hip) share, and the one header each of them starts from: it
// brings the grid helpers (cn_common.hpp), the accumulation primitive (cn_det.hpp) and the gradient scatter (grid_scatter.hpp),
// and adds the 64-sample tile constants of the scalar, tile and wave kernels, the by-value kernel arguments of the two entry
// families, and the SH derivative.
#pragma once

#include "cn_common.hpp"
#include "cn_det.hpp"
#include "grid_scatter.hpp"

namespace cn {

constexpr int TS = 64;       // samples per tile
constexpr int LD = TS + 1;   // padded row length
constexpr int TB = 256;      // threads per workgroup

struct FieldPtrs {
  const float* table;
  const float *w0, *b0, *w1, *b1;
  const float *ws0, *bs0, *ws1, *bs1, *wh, *bh;
  const float *wc0, *bc0, *wc1, *bc1, *wc2, *bc2;
  const float* emb;
};
struct FieldGrads {
  float* table;
  float *w0, *b0, *w1, *b1;
  float *ws0, *bs0, *ws1, *bs1, *wh, *bh;
  float *wc0, *bc0, *wc1, *bc1, *wc2, *bc2;
  float* emb;
};

struct FieldBwdArgs {
  FieldPtrs p;
  FieldGrads g;
  GridDev grid;  // geometry of p.table / g.table (fp32 tables)
  SceneDev scene;
  int sh_unit;
  int app_per_camera;
  const float* app_mean;  // [32] when not per-camera (may be null -> zeros)
  const float *origins, *directions, *starts, *ends;
  const int64_t* cam_idx;
  const float *d_density, *d_rgb, *d_sem;
  long long R;
  int S;
  float *d_pos, *d_dir;  // optional [R*S,3] outputs for the camera pose refinement (null: skipped)
  CoarseScatter coarse;  // private copies for level 0's gradient (cn_grid.scatter_scratch of the gradient grid)
  CellScatter cells;     // cell-major records of the coarse levels (take precedence for the levels they cover)
};

struct PropBwdArgs {
  const float* table;
  const float *w0, *b0, *w1, *b1;
  float *g_table, *g_w0, *g_b0, *g_w1, *g_b1;
  GridDev grid;
  SceneDev scene;
  const float *origins, *directions, *starts, *ends, *d_density;
  float* d_pos;  // optional [R*S,3]
  long long R;
  int S;
  CoarseScatter coarse;
  CellScatter cells;  // cell-major records of the coarse levels (takes precedence over `coarse` for the levels it covers)
};

// d SH_deg4 / d (x, y, z) contracted with g[16] (the derivative of sh_deg4 in cn_common.hpp, term by term)
__device__ __forceinline__ void sh_deg4_backward(float x, float y, float z, const float* g, float& dx, float& dy,
                                                 float& dz) {
  const float xx = x * x, yy = y * y, zz = z * z;
  dx = 0.4886025119029199f * g[3] + 1.0925484305920792f * (y * g[4] + z * g[7]) + 1.0925484305920792f * x * g[8] +
       0.5900435899266435f * 6.f * x * y * g[9] + 2.890611442640554f * y * z * g[10] +
       0.4570457994644658f * (5.f * zz - 1.f) * g[13] + 1.445305721320277f * 2.f * x * z * g[14] +
       0.5900435899266435f * 3.f * (xx - yy) * g[15];
  dy = 0.4886025119029199f * g[1] + 1.0925484305920792f * (x * g[4] + z * g[5]) - 1.0925484305920792f * y * g[8] +
       0.5900435899266435f * 3.f * (xx - yy) * g[9] + 2.890611442640554f * x * z * g[10] +
       0.4570457994644658f * (5.f * zz - 1.f) * g[11] - 1.445305721320277f * 2.f * y * z * g[14] -
       0.5900435899266435f * 6.f * x * y * g[15];
  dz = 0.4886025119029199f * g[2] + 1.0925484305920792f * (y * g[5] + x * g[7]) + 0.9461746957575601f * 2.f * z * g[6] +
       2.890611442640554f * x * y * g[10] + 0.4570457994644658f * 10.f * z * (y * g[11] + x * g[13]) +
       0.3731763325901154f * (15.f * zz - 3.f) * g[12] + 1.445305721320277f * (xx - yy) * g[14];
}

}  // namespace cn
