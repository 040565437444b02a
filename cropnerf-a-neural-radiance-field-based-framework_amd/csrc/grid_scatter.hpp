// The hash-grid gradient scatter of the training backward kernels (train_field.hip): how d loss / d (a level's features)
// reaches the gradient table.  Everything about it lives here:
//   * the scratch layouts behind cn_grid.scatter_scratch -- CoarseScatter (private dense copies of level 0) and CellScatter
//     (cell-major records of the coarse levels) -- and the host functions that lay them out;
//   * the per-level device routines the backward kernels call: hash_level_backward (table path), _private, _cells, _cells_rows;
//   * the kernels that fold the scratch into the table afterwards, and their launchers;
//   * the host-side plan / finish pair every backward entry point brackets its kernel with.
// The four hash_level_backward* forms and the two fold kernels repeat each other in places on purpose: see the note on
// moving versus rewriting device code in DESIGN.md before merging them.
#pragma once

#include <cstdlib>

#include "cn_common.hpp"
#include "cn_det.hpp"

namespace cn {

// Private accumulation of the coarsest level's gradient (cn_grid.scatter_scratch): `copies` dense [n1^3][2] arrays,
// vertex (x, y, z) at x + n1 * (y + n1 * z); a workgroup adds to copy blockIdx.x % copies.  base == nullptr: off.
struct CoarseScatter {
  float* base;
  unsigned n1, copies;
};
constexpr unsigned COARSE_COPIES = 64, COARSE_MIN_COPIES = 8, COARSE_MAX_N1 = 40;
// vertices per axis that level 0 can address for positions in [0, 1]: floor(scale + offset) is the largest cell index
inline unsigned coarse_n1(const cn_grid& g) {
  const float off = g.layout == CN_GRID_TCNN ? 0.5f : 0.f;
  return (unsigned)floorf(g.scalings[0] + off) + 2u;
}
inline CoarseScatter make_coarse_scatter(const cn_grid& grads_grid) {
  CoarseScatter c{nullptr, 0u, 0u};
  if (!grads_grid.scatter_scratch || grads_grid.num_levels < 1) return c;
  const unsigned n1 = coarse_n1(grads_grid);
  if (n1 > COARSE_MAX_N1) return c;
  const size_t per_copy = (size_t)n1 * n1 * n1 * 2 * sizeof(float);
  size_t copies = grads_grid.scatter_scratch_bytes / per_copy;
  if (copies > COARSE_COPIES) copies = COARSE_COPIES;
  if (copies < COARSE_MIN_COPIES) return c;
  c.base = static_cast<float*>(grads_grid.scatter_scratch);
  c.n1 = n1;
  c.copies = (unsigned)copies;
  return c;
}

// Cell-major gradient records of the coarse levels (cn_grid.scatter_scratch, behind the level-0 vertex copies): level l < num_levels
// keeps copies[l] arrays of n[l]^3 records of 16 floats -- the 8 corners x 2 features of ONE cell, corner c = a + 2 b + 4 d at
// floats 2c, 2c + 1 -- so that a sample adds its whole cell in ONE 64-byte request (the hash table takes 4.5: one per x-edge),
// and consecutive samples of a ray in the same cell merge into one.  A fold kernel adds the touched records to the table and
// zeroes them.  Worth it where samples outnumber cells: the launch picks the levels by batch size.
constexpr int CN_CELL_LEVELS = 10;
// A level goes through cell-major records when it has at most (ratio x samples of the call) cells.  Since the fold works by
// blocks (cell_scatter_fold_blocks_kernel: ~0.4 requests per cell and a streaming pass over the records) a level pays as long as
// one request per run of samples plus that pass is cheaper than 4.5 requests per sample: measured optimum (tools/train_probe.py,
// 4 096 / 65 536 rays) at ~2-3 cells per sample for the field (48 samples per ray: few samples share a cell at the
// fine levels; 3.03 -- 9.5e6 cells, 610 MB of records at 65 536 rays -- already costs 0.6 ms) and 3-8 for the proposal networks
// (256 / 96 samples per ray: runs merge).  CELL_RATIO_MAX bounds what cn_grid_scatter_scratch_bytes_for sizes the scratch for.
constexpr double CELL_RATIO_FIELD = 2.85, CELL_RATIO_PROPOSAL = 6.0, CELL_RATIO_MAX = 8.0;
constexpr unsigned long long CELL_MAX_CELLS = 17500000ull;  // 259^3 fits
struct CellScatter {
  float* base;  // nullptr: off
  int num_levels;
  unsigned n[CN_CELL_LEVELS];
  unsigned copies[CN_CELL_LEVELS];
  unsigned long long offset[CN_CELL_LEVELS];  // in floats from base
};
inline unsigned cell_n(const cn_grid& g, int l) {  // cells per axis that positions in [0, 1] can fall into
  const float off = g.layout == CN_GRID_TCNN ? 0.5f : 0.f;
  return (unsigned)floorf(g.scalings[l] + off) + 1u;
}
inline unsigned cell_copies(unsigned long long ncells) { return ncells <= 8192 ? 16u : ncells <= 65536 ? 4u : 1u; }
// bytes of the vertex copies (first part of the scratch)
inline size_t coarse_scratch_bytes(const cn_grid& g) {
  if (g.num_levels < 1) return 0;
  const unsigned n1 = coarse_n1(g);
  return n1 > COARSE_MAX_N1 ? 0 : (size_t)COARSE_COPIES * n1 * n1 * n1 * 2 * sizeof(float);
}
// the consecutive coarse levels that may be kept cell-major, and the bytes they need (second part of the scratch)
inline size_t cell_scratch_layout(const cn_grid& g, CellScatter* out) {
  CellScatter c{};
  unsigned long long floats = 0;
  for (int l = 0; l < g.num_levels && l < CN_CELL_LEVELS; ++l) {
    const unsigned n = cell_n(g, l);
    const unsigned long long cells = (unsigned long long)n * n * n;
    if (cells > CELL_MAX_CELLS) break;
    c.n[l] = n;
    c.copies[l] = cell_copies(cells);
    c.offset[l] = floats;
    floats += c.copies[l] * cells * 16ull;
    c.num_levels = l + 1;
  }
  if (out) *out = c;
  return (size_t)floats * sizeof(float);
}
// levels 0 .. k-1 with at most max_cells cells each (the launch passes ratio x samples).  Of a small level's copies only as
// many are used as the batch needs to keep the requests per record in the low hundreds: ~ samples / (48 cells), rounded up
// to a power of two.
inline CellScatter make_cell_scatter(const cn_grid& grads_grid, unsigned long long max_cells, unsigned long long samples) {
  CellScatter c{};
  if (!grads_grid.scatter_scratch) return c;
  const size_t head = coarse_scratch_bytes(grads_grid);
  const size_t need = cell_scratch_layout(grads_grid, &c);
  if (need == 0 || grads_grid.scatter_scratch_bytes < head) {
    c = CellScatter{};
    return c;
  }
  // the scratch may hold a PREFIX of the levels (cn_grid_scatter_scratch_bytes_for: sized for a maximum batch): use the
  // levels whose records fit it
  int fit = 0;
  while (fit < c.num_levels) {
    const unsigned long long cells = (unsigned long long)c.n[fit] * c.n[fit] * c.n[fit];
    const unsigned long long end = (c.offset[fit] + c.copies[fit] * cells * 16ull) * sizeof(float);
    if (head + end > grads_grid.scatter_scratch_bytes) break;
    ++fit;
  }
  c.num_levels = fit;
  int k = 0;
  while (k < c.num_levels && (unsigned long long)c.n[k] * c.n[k] * c.n[k] <= max_cells) ++k;
  c.num_levels = k;
  for (int l = 0; l < k; ++l) {
    const unsigned long long cells = (unsigned long long)c.n[l] * c.n[l] * c.n[l];
    unsigned want = 1;
    while (want < c.copies[l] && (unsigned long long)want * cells * 48ull < samples) want <<= 1;
    c.copies[l] = want;
  }
  c.base = k > 0 ? reinterpret_cast<float*>(static_cast<char*>(grads_grid.scatter_scratch) + head) : nullptr;
  return c;
}

__device__ __forceinline__ unsigned cell_n_of(const CellScatter& c, int l) {
  unsigned v = c.n[0];
#pragma unroll
  for (int k = 1; k < CN_CELL_LEVELS; ++k) v = l == k ? c.n[k] : v;
  return v;
}
__device__ __forceinline__ unsigned cell_copies_of(const CellScatter& c, int l) {
  unsigned v = c.copies[0];
#pragma unroll
  for (int k = 1; k < CN_CELL_LEVELS; ++k) v = l == k ? c.copies[k] : v;
  return v;
}
__device__ __forceinline__ unsigned long long cell_offset_of(const CellScatter& c, int l) {
  unsigned long long v = c.offset[0];
#pragma unroll
  for (int k = 1; k < CN_CELL_LEVELS; ++k) v = l == k ? c.offset[k] : v;
  return v;
}

// Run-length pre-reduction of scatter-adds inside each 16-lane row.  Lanes are consecutive samples of a ray, so at the
// coarser levels neighbouring lanes hit the same grid cell: runs of equal `key` are summed with a segmented scan on DPP
// row shifts (no LDS, no address registers) and only the last lane of a run issues the atomic.  Must be called by all
// 64 lanes (pass zeros for lanes with nothing to add).  Returns true where the (summed) v0 / v1 are to be added.
template <int CTRL>
__device__ __forceinline__ unsigned dpp_u32(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ bool row_run_reduce(unsigned key, float& v0, float& v1, int row_lane) {
  const unsigned prev = dpp_u32<0x111>(key);  // row_shr:1
  unsigned head = (row_lane == 0 || prev != key) ? 1u : 0u;
  const unsigned next_head = dpp_u32<0x101>(head);  // row_shl:1 (0 past the row end)
  const bool last = row_lane == 15 || next_head != 0u;
  unsigned f = head;
#define CN_SEG_STEP(CTRL)                         \
  {                                               \
    const float a0 = dpp_f32<CTRL>(v0);           \
    const float a1 = dpp_f32<CTRL>(v1);           \
    const unsigned fu = dpp_u32<CTRL>(f);         \
    if (!f) {                                     \
      v0 += a0;                                   \
      v1 += a1;                                   \
      f |= fu;                                    \
    }                                             \
  }
  CN_SEG_STEP(0x111)
  CN_SEG_STEP(0x112)
  CN_SEG_STEP(0x114)
  CN_SEG_STEP(0x118)
#undef CN_SEG_STEP
  return last;
}

// scatter d(loss)/d(features of one level) into the table gradient with the forward's trilinear weights
// (all 64 lanes call it; g0 = g1 = 0 for lanes without a sample).  POS: also accumulate d(loss)/d(normalised position)
// -- the trilinear weights are linear in the in-cell offset, so d enc_f / d x = scale * sum_c (+-1) wy wz table[c].f
// (the path HashEncoding.pytorch_fwd's `offset = scaled - floor(scaled)` carries gradient through; it is what feeds
// the camera pose refinement).
template <bool POS>
__device__ __forceinline__ void hash_level_backward(float* __restrict__ gtab, const float* __restrict__ table,
                                                    const Lvl& lv, float pos_offset, float px, float py, float pz,
                                                    float g0, float g1, int lane, float& dpx, float& dpy, float& dpz) {
  const Cell cell = hash_cell(lv, pos_offset, px, py, pz);
  const float ox = cell.ox, oy = cell.oy, oz = cell.oz, scale = lv.scale;
  const unsigned mask = lv.mask, level_off = lv.off;
  unsigned hx[2] = {cell.hx0, cell.hx1};
  unsigned hy[2] = {cell.hy0, cell.hy1};
  unsigned hz[2] = {cell.hz0, cell.hz1};
  float wx[2] = {1.f - ox, ox}, wy[2] = {1.f - oy, oy}, wz[2] = {1.f - oz, oz};  // index 1 = ceil corner
  const int row_lane = lane & 15;
  float ax = 0.f, ay = 0.f, az = 0.f;
  // The index xors ix into the low bits (hashed and dense levels alike), so the two corners of an x-edge lie in one
  // aligned 64-byte segment of the table unless ix = 7 (mod 8) -- and the memory pipe takes everything ONE instruction sends to one 64-byte segment as ONE
  // atomic request, whatever the lanes (tools/atomic_microbench.hip: 21e9 requests/s, the bound of this kernel).  Each
  // atomic instruction therefore serves ONE x-edge of one source lane from FOUR adjacent lanes (entry = lane & 2 ? x1
  // corner : x0 corner, feature = lane & 1); the four source lanes of a quad take turns: 4 requests per sample and
  // level for 7 of 8 cells instead of 16 single floats.
#pragma unroll
  for (int bd = 0; bd < 4; ++bd) {
    const int b = bd & 1, d = bd >> 1;
    unsigned eu[2];
    float v0[2], v1[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const float w = wx[a] * wy[b] * wz[d];
      const unsigned e = ((hx[a] ^ hy[b] ^ hz[d]) & mask) + level_off;
      if constexpr (POS) {
        const float2 t = hash_gather(table, e);
        const float tg = t.x * g0 + t.y * g1;
        ax += (a ? tg : -tg) * (wy[b] * wz[d]);
        ay += (b ? tg : -tg) * (wx[a] * wz[d]);
        az += (d ? tg : -tg) * (wx[a] * wy[b]);
      }
      v0[a] = w * g0;
      v1[a] = w * g1;
      const bool issue = row_run_reduce(e, v0[a], v1[a], row_lane);
      eu[a] = issue && (v0[a] != 0.f || v1[a] != 0.f) ? e : 0xffffffffu;
    }
    const int ql = lane & 3;
#define CN_QUAD_ROUND(CTRL)                                                                          \
  {                                                                                                  \
    const unsigned e0 = dpp_u32<CTRL>(eu[0]), e1 = dpp_u32<CTRL>(eu[1]);                             \
    const float a00 = dpp_f32<CTRL>(v0[0]), a01 = dpp_f32<CTRL>(v1[0]);                              \
    const float a10 = dpp_f32<CTRL>(v0[1]), a11 = dpp_f32<CTRL>(v1[1]);                              \
    const unsigned es = (ql & 2) ? e1 : e0;                                                          \
    const float val = (ql & 2) ? ((ql & 1) ? a11 : a10) : ((ql & 1) ? a01 : a00);                    \
    if (es != 0xffffffffu) cn_atomic_add(gtab + 2 * (size_t)es + (ql & 1), val);                         \
  }
    CN_QUAD_ROUND(0x00)  // quad_perm [0,0,0,0]
    CN_QUAD_ROUND(0x55)  // [1,1,1,1]
    CN_QUAD_ROUND(0xAA)  // [2,2,2,2]
    CN_QUAD_ROUND(0xFF)  // [3,3,3,3]
#undef CN_QUAD_ROUND
  }
  // (History, measured at 4096 rays: one atomic per float from the owning lane 2.73 ms; the two features of an entry from
  // two adjacent lanes of one instruction 1.73 ms; this x-edge form 1.30 ms.  The earlier forms were removed.)
  if constexpr (POS) {
    dpx = fmaf(ax, scale, dpx);
    dpy = fmaf(ay, scale, dpy);
    dpz = fmaf(az, scale, dpz);
  }
}

// The same for the level whose gradient is accumulated in private dense copies (CoarseScatter): the atomics go to
// `priv` (this workgroup's copy) at the vertex's dense index; lanes whose cell lies outside the copy's n1^3 vertices
// (positions outside [0, 1]: only without scene contraction) take the table path afterwards.  The position gradient reads
// the parameter table at the real entries as before.
template <bool POS>
__device__ __forceinline__ void hash_level_backward_private(float* __restrict__ priv, unsigned n1,
                                                            float* __restrict__ gtab, const float* __restrict__ table,
                                                            const Lvl& lv, float pos_offset, float px, float py, float pz,
                                                            float g0, float g1, int lane, float& dpx, float& dpy,
                                                            float& dpz) {
  const Cell cell = hash_cell(lv, pos_offset, px, py, pz);
  const float ox = cell.ox, oy = cell.oy, oz = cell.oz, scale = lv.scale;
  // the integer cell coordinates again (hash_cell keeps their index terms only)
  const unsigned ix = cell.hx0;
  const unsigned iy = (unsigned)(int)floorf(fmaf(py, lv.scale, pos_offset));
  const unsigned iz = (unsigned)(int)floorf(fmaf(pz, lv.scale, pos_offset));
  const bool inside = ix + 1u < n1 && iy + 1u < n1 && iz + 1u < n1;  // unsigned: negative coordinates are huge
  const float h0 = inside ? g0 : 0.f, h1 = inside ? g1 : 0.f;
  unsigned hx[2] = {cell.hx0, cell.hx1};
  unsigned hy[2] = {cell.hy0, cell.hy1};
  unsigned hz[2] = {cell.hz0, cell.hz1};
  float wx[2] = {1.f - ox, ox}, wy[2] = {1.f - oy, oy}, wz[2] = {1.f - oz, oz};
  const int row_lane = lane & 15;
  float ax = 0.f, ay = 0.f, az = 0.f;
#pragma unroll
  for (int bd = 0; bd < 4; ++bd) {
    const int b = bd & 1, d = bd >> 1;
    unsigned eu[2];
    float v0[2], v1[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const float w = wx[a] * wy[b] * wz[d];
      const unsigned e = inside ? (ix + a) + n1 * ((iy + b) + n1 * (iz + d)) : 0xfffffffeu;
      if constexpr (POS) {
        const float2 t = hash_gather(table, ((hx[a] ^ hy[b] ^ hz[d]) & lv.mask) + lv.off);
        const float tg = t.x * h0 + t.y * h1;
        ax += (a ? tg : -tg) * (wy[b] * wz[d]);
        ay += (b ? tg : -tg) * (wx[a] * wz[d]);
        az += (d ? tg : -tg) * (wx[a] * wy[b]);
      }
      v0[a] = w * h0;
      v1[a] = w * h1;
      const bool issue = row_run_reduce(e, v0[a], v1[a], row_lane);
      eu[a] = issue && (v0[a] != 0.f || v1[a] != 0.f) ? e : 0xffffffffu;
    }
    const int ql = lane & 3;
#define CN_QUAD_ROUND(CTRL)                                                                          \
  {                                                                                                  \
    const unsigned e0 = dpp_u32<CTRL>(eu[0]), e1 = dpp_u32<CTRL>(eu[1]);                             \
    const float a00 = dpp_f32<CTRL>(v0[0]), a01 = dpp_f32<CTRL>(v1[0]);                              \
    const float a10 = dpp_f32<CTRL>(v0[1]), a11 = dpp_f32<CTRL>(v1[1]);                              \
    const unsigned es = (ql & 2) ? e1 : e0;                                                          \
    const float val = (ql & 2) ? ((ql & 1) ? a11 : a10) : ((ql & 1) ? a01 : a00);                    \
    if (es != 0xffffffffu) cn_atomic_add(priv + 2 * (size_t)es + (ql & 1), val);                         \
  }
    CN_QUAD_ROUND(0x00)
    CN_QUAD_ROUND(0x55)
    CN_QUAD_ROUND(0xAA)
    CN_QUAD_ROUND(0xFF)
#undef CN_QUAD_ROUND
  }
  if constexpr (POS) {
    dpx = fmaf(ax, scale, dpx);
    dpy = fmaf(ay, scale, dpy);
    dpz = fmaf(az, scale, dpz);
  }
  // cells outside the private copy (never with scene contraction): the plain path, for those lanes only
  if (__builtin_amdgcn_ballot_w64(!inside && (g0 != 0.f || g1 != 0.f)) != 0ull)
    hash_level_backward<POS>(gtab, table, lv, pos_offset, px, py, pz, inside ? 0.f : g0, inside ? 0.f : g1, lane, dpx, dpy,
                             dpz);
}

// The scatter of one CELL-MAJOR level (CellScatter): every sample adds the 16 weighted values of its cell -- 8 corners x 2
// features -- to the cell's 64-byte record with ONE request: runs of consecutive samples in the same cell are summed first
// (the same DPP run-length reduction, keyed by the cell), the 16 sums of a run end go through a wave-private LDS buffer
// `tb` ([64][17] floats) so that 16 lanes carry one record, and in round k the 16 lanes of every row add the record of the
// row's k-th sample.  Cells outside the n^3 array (positions outside [0, 1]: only without scene contraction) take the table
// path afterwards.  All 64 lanes of the wave must call.
template <bool POS>
__device__ __forceinline__ void hash_level_backward_cells(float* __restrict__ rec, unsigned n, float* __restrict__ tb,
                                                          float* __restrict__ gtab, const float* __restrict__ table,
                                                          const Lvl& lv, float pos_offset, float px, float py, float pz,
                                                          float g0, float g1, int lane, float& dpx, float& dpy,
                                                          float& dpz) {
  const Cell cell = hash_cell(lv, pos_offset, px, py, pz);
  const float ox = cell.ox, oy = cell.oy, oz = cell.oz;
  const unsigned ix = cell.hx0;
  const unsigned iy = (unsigned)(int)floorf(fmaf(py, lv.scale, pos_offset));
  const unsigned iz = (unsigned)(int)floorf(fmaf(pz, lv.scale, pos_offset));
  const bool inside = ix < n && iy < n && iz < n;  // unsigned: negative coordinates are huge
  const float h0 = inside ? g0 : 0.f, h1 = inside ? g1 : 0.f;
  const unsigned key = inside ? ix + n * (iy + n * iz) : 0xfffffffeu;
  const float wx[2] = {1.f - ox, ox}, wy[2] = {1.f - oy, oy}, wz[2] = {1.f - oz, oz};
  const int row_lane = lane & 15;
  bool last = false, any = false;
  float ax = 0.f, ay = 0.f, az = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int a = c & 1, b = (c >> 1) & 1, d = c >> 2;
    const float w = wx[a] * wy[b] * wz[d];
    if constexpr (POS) {
      const unsigned hx = a ? cell.hx1 : cell.hx0, hy = b ? cell.hy1 : cell.hy0, hz = d ? cell.hz1 : cell.hz0;
      const float2 t = hash_gather(table, ((hx ^ hy ^ hz) & lv.mask) + lv.off);
      const float tg = t.x * h0 + t.y * h1;
      ax += (a ? tg : -tg) * (wy[b] * wz[d]);
      ay += (b ? tg : -tg) * (wx[a] * wz[d]);
      az += (d ? tg : -tg) * (wx[a] * wy[b]);
    }
    float v0 = w * h0, v1 = w * h1;
    last = row_run_reduce(key, v0, v1, row_lane);
    any = any || v0 != 0.f || v1 != 0.f;
    tb[lane * 17 + 2 * c] = v0;
    tb[lane * 17 + 2 * c + 1] = v1;
  }
  tb[lane * 17 + 16] = __builtin_bit_cast(float, (last && any && inside) ? key : 0xffffffffu);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int row0 = lane & 48;
#pragma unroll 4
  for (int k = 0; k < 16; ++k) {
    const unsigned cellk = __builtin_bit_cast(unsigned, tb[(row0 + k) * 17 + 16]);
    if (cellk != 0xffffffffu) cn_atomic_add(rec + (size_t)cellk * 16 + row_lane, tb[(row0 + k) * 17 + row_lane]);
  }
  __builtin_amdgcn_wave_barrier();
  if constexpr (POS) {
    dpx = fmaf(ax, lv.scale, dpx);
    dpy = fmaf(ay, lv.scale, dpy);
    dpz = fmaf(az, lv.scale, dpz);
  }
  if (__builtin_amdgcn_ballot_w64(!inside && (g0 != 0.f || g1 != 0.f)) != 0ull)
    hash_level_backward<POS>(gtab, table, lv, pos_offset, px, py, pz, inside ? 0.f : g0, inside ? 0.f : g1, lane, dpx, dpy,
                             dpz);
}

// hash_level_backward_cells with the run-length reduction done AFTER the transpose: every lane writes its 16 weighted values
// and its cell to the wave-private buffer unreduced; then the 16 lanes of a row walk the row's 16 samples in order, each lane
// summing one of the 16 record entries, and add the sum to the cell's record whenever the next sample lies in another cell.
// Same requests as the DPP form (one per run of samples in a cell), a third of its instructions: no segmented scans -- 16
// values x 4 steps of cross-lane moves -- only a running sum.  The sums of a run are taken in sample order instead of as a
// tree, so the last bit may differ from the first form's.  All 64 lanes must call; gradient only (no position gradient).
__device__ __forceinline__ void hash_level_backward_cells_rows(float* __restrict__ rec, unsigned n, float* __restrict__ tb,
                                                               float* __restrict__ gtab, const float* __restrict__ table,
                                                               const Lvl& lv, float pos_offset, float px, float py, float pz,
                                                               float g0, float g1, int lane) {
  const Cell cell = hash_cell(lv, pos_offset, px, py, pz);
  const float ox = cell.ox, oy = cell.oy, oz = cell.oz;
  const unsigned ix = cell.hx0;
  const unsigned iy = (unsigned)(int)floorf(fmaf(py, lv.scale, pos_offset));
  const unsigned iz = (unsigned)(int)floorf(fmaf(pz, lv.scale, pos_offset));
  const bool inside = ix < n && iy < n && iz < n;  // unsigned: negative coordinates are huge
  const float h0 = inside ? g0 : 0.f, h1 = inside ? g1 : 0.f;
  const float wx[2] = {1.f - ox, ox}, wy[2] = {1.f - oy, oy}, wz[2] = {1.f - oz, oz};
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float w = wx[c & 1] * wy[(c >> 1) & 1] * wz[c >> 2];
    tb[lane * 17 + 2 * c] = w * h0;
    tb[lane * 17 + 2 * c + 1] = w * h1;
  }
  tb[lane * 17 + 16] = __builtin_bit_cast(float, inside ? ix + n * (iy + n * iz) : 0xffffffffu);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int row0 = lane & 48, row_lane = lane & 15;
  float acc = 0.f;
  unsigned cur = __builtin_bit_cast(unsigned, tb[row0 * 17 + 16]);
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    acc += tb[(row0 + k) * 17 + row_lane];
    const unsigned next = k < 15 ? __builtin_bit_cast(unsigned, tb[(row0 + k + 1) * 17 + 16]) : 0xfffffffdu;
    if (next != cur) {  // (uniform within the row)
      if (cur != 0xffffffffu && acc != 0.f) cn_atomic_add(rec + (size_t)cur * 16 + row_lane, acc);
      acc = 0.f;
    }
    cur = next;
  }
  __builtin_amdgcn_wave_barrier();
  if (__builtin_amdgcn_ballot_w64(!inside && (g0 != 0.f || g1 != 0.f)) != 0ull) {
    float ux = 0.f, uy = 0.f, uz = 0.f;
    hash_level_backward<false>(gtab, table, lv, pos_offset, px, py, pz, inside ? 0.f : g0, inside ? 0.f : g1, lane, ux, uy, uz);
  }
}

#if CN_DETERMINISTIC_SCATTER
// fold the cell-major levels into the gradient table and zero their touched records: one thread per (copy, cell) record,
// all levels in one launch (workgroups [first_block[l], first_block[l + 1]) belong to level l).  Only the deterministic
// build compiles it: the block form below sums in LDS with float atomics of four waves, in no fixed order.
struct CellFoldArgs {
  CellScatter c;
  unsigned first_block[CN_CELL_LEVELS + 1];
  Lvl lv[CN_CELL_LEVELS];
};
__global__ void __launch_bounds__(256) cell_scatter_fold_kernel(CellFoldArgs F, float* __restrict__ gtab) {
  int l = 0;
#pragma unroll
  for (int k = 1; k < CN_CELL_LEVELS; ++k) l = (k < F.c.num_levels && blockIdx.x >= F.first_block[k]) ? k : l;  // block-uniform
  unsigned n = F.c.n[0], copies = F.c.copies[0], first = F.first_block[0];
  unsigned long long off = F.c.offset[0];
  Lvl lv = F.lv[0];
#pragma unroll
  for (int k = 1; k < CN_CELL_LEVELS; ++k) {
    const bool m = l == k;
    n = m ? F.c.n[k] : n;
    copies = m ? F.c.copies[k] : copies;
    first = m ? F.first_block[k] : first;
    off = m ? F.c.offset[k] : off;
    lv.off = m ? F.lv[k].off : lv.off;
    lv.mask = m ? F.lv[k].mask : lv.mask;
    lv.m1 = m ? F.lv[k].m1 : lv.m1;
    lv.m2 = m ? F.lv[k].m2 : lv.m2;
  }
  const unsigned long long cells = (unsigned long long)n * n * n;
  const unsigned long long i = (blockIdx.x - first) * 256ull + threadIdx.x;
  if (i >= cells * copies) return;
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  f32x4* p = reinterpret_cast<f32x4*>(F.c.base + off + i * 16);
  const f32x4 r0 = p[0], r1 = p[1], r2 = p[2], r3 = p[3];
  const float v[16] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w};
  bool any = false;
#pragma unroll
  for (int j = 0; j < 16; ++j) any = any || v[j] != 0.f;
  if (!any) return;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  p[0] = zero;
  p[1] = zero;
  p[2] = zero;
  p[3] = zero;
  const unsigned long long cidx = i % cells;
  const unsigned x = (unsigned)(cidx % n), y = (unsigned)((cidx / n) % n), z = (unsigned)(cidx / ((unsigned long long)n * n));
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    if (v[2 * c] == 0.f && v[2 * c + 1] == 0.f) continue;
    const unsigned e = (((x + (c & 1)) ^ ((y + ((c >> 1) & 1)) * lv.m1) ^ ((z + (c >> 2)) * lv.m2)) & lv.mask) + lv.off;
    cn_atomic_add(gtab + 2 * (size_t)e, v[2 * c]);
    cn_atomic_add(gtab + 2 * (size_t)e + 1, v[2 * c + 1]);
  }
}
#else
// The product build's fold, by BLOCKS of 8 x 8 x 8 cells (round 4).  The per-record form adds every touched record's 16
// values to the table one float per atomic instruction: up to 16 requests per record and copy, 4.3e6 per call at 65 536
// rays -- the fold was bound by its own atomics (0.27 ms per call, three calls per iteration).  Here a workgroup owns a block of cells in up to four of
// the level's copies, sums their records into the block's 9 x 9 x 9 vertices in LDS (ds_add_f32), and then adds every non-zero
// vertex to the table ONCE, two lanes per vertex (its two features) and vertices in x order: the index function xors x into
// the low bits, so the eight vertices of an aligned x-row of the block lie on one 64-byte line and travel as one request.
// Requests per block: ~2 per (y, z) row of vertices instead of up to 16 per record.
struct CellFoldBlocksArgs {
  CellScatter c;
  unsigned first_block[CN_CELL_LEVELS + 1];
  unsigned nb[CN_CELL_LEVELS];      // blocks per axis
  unsigned groups[CN_CELL_LEVELS];  // workgroups per block: the level's copies are dealt out over them
  Lvl lv[CN_CELL_LEVELS];
};
__global__ void __launch_bounds__(256) cell_scatter_fold_blocks_kernel(CellFoldBlocksArgs F, float* __restrict__ gtab) {
  __shared__ float acc[2 * 729];
  int l = 0;
#pragma unroll
  for (int k = 1; k < CN_CELL_LEVELS; ++k) l = (k < F.c.num_levels && blockIdx.x >= F.first_block[k]) ? k : l;  // block-uniform
  unsigned n = F.c.n[0], copies = F.c.copies[0], first = F.first_block[0], nb = F.nb[0], groups = F.groups[0];
  unsigned long long off = F.c.offset[0];
  Lvl lv = F.lv[0];
#pragma unroll
  for (int k = 1; k < CN_CELL_LEVELS; ++k) {
    const bool m = l == k;
    n = m ? F.c.n[k] : n;
    copies = m ? F.c.copies[k] : copies;
    first = m ? F.first_block[k] : first;
    nb = m ? F.nb[k] : nb;
    groups = m ? F.groups[k] : groups;
    off = m ? F.c.offset[k] : off;
    lv.off = m ? F.lv[k].off : lv.off;
    lv.mask = m ? F.lv[k].mask : lv.mask;
    lv.m1 = m ? F.lv[k].m1 : lv.m1;
    lv.m2 = m ? F.lv[k].m2 : lv.m2;
  }
  const int tid = threadIdx.x;
  for (int i = tid; i < 2 * 729; i += 256) acc[i] = 0.f;
  __syncthreads();
  const unsigned local = blockIdx.x - first, grp = local % groups, b = local / groups;
  const unsigned bx = b % nb, by = (b / nb) % nb, bz = b / (nb * nb);
  const unsigned long long cells = (unsigned long long)n * n * n;
  typedef float f32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const unsigned cl = tid + 256 * h, lx = cl & 7u, ly = (cl >> 3) & 7u, lz = cl >> 6;
    const unsigned x = bx * 8 + lx, y = by * 8 + ly, z = bz * 8 + lz;
    if (x >= n || y >= n || z >= n) continue;
    const unsigned long long cidx = x + (unsigned long long)n * (y + (unsigned long long)n * z);
    for (unsigned k = grp; k < copies; k += groups) {
      f32x4* p = reinterpret_cast<f32x4*>(F.c.base + off + ((unsigned long long)k * cells + cidx) * 16);
      const f32x4 r0 = p[0], r1 = p[1], r2 = p[2], r3 = p[3];
      const float v[16] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w};
      bool any = false;
#pragma unroll
      for (int j = 0; j < 16; ++j) any = any || v[j] != 0.f;
      if (!any) continue;
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
      p[0] = zero;
      p[1] = zero;
      p[2] = zero;
      p[3] = zero;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const unsigned vi = ((lz + (c >> 2)) * 9 + (ly + ((c >> 1) & 1))) * 9 + (lx + (c & 1));
        if (v[2 * c] != 0.f) atomicAdd(&acc[2 * vi], v[2 * c]);
        if (v[2 * c + 1] != 0.f) atomicAdd(&acc[2 * vi + 1], v[2 * c + 1]);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < 2 * 729; i += 256) {
    const float val = acc[i];
    if (val == 0.f) continue;
    const unsigned vtx = (unsigned)i >> 1, vx = vtx % 9, vy = (vtx / 9) % 9, vz = vtx / 81;
    const unsigned e = (((bx * 8 + vx) ^ ((by * 8 + vy) * lv.m1) ^ ((bz * 8 + vz) * lv.m2)) & lv.mask) + lv.off;
    cn_atomic_add(gtab + 2 * (size_t)e + (i & 1), val);
  }
}
#endif
inline void launch_cell_fold(const CellScatter& c, const GridDev& grid, float* gtab, hipStream_t stream) {
  if (!c.base || c.num_levels <= 0) return;
#if CN_DETERMINISTIC_SCATTER
  CellFoldArgs F{};
  F.c = c;
  unsigned blocks = 0;
  for (int l = 0; l < c.num_levels; ++l) {
    F.first_block[l] = blocks;
    F.lv[l] = grid.level(l);
    const unsigned long long recs = (unsigned long long)c.n[l] * c.n[l] * c.n[l] * c.copies[l];
    blocks += (unsigned)((recs + 255) / 256);
  }
  for (int l = c.num_levels; l <= CN_CELL_LEVELS; ++l) F.first_block[l] = blocks;
  hipLaunchKernelGGL(cell_scatter_fold_kernel, dim3(blocks), dim3(256), 0, stream, F, gtab);
#else
  CellFoldBlocksArgs B{};
  B.c = c;
  unsigned blocks = 0;
  for (int l = 0; l < c.num_levels; ++l) {
    B.first_block[l] = blocks;
    B.lv[l] = grid.level(l);
    B.nb[l] = (c.n[l] + 7) / 8;
    B.groups[l] = (c.copies[l] + 3) / 4;
    blocks += B.nb[l] * B.nb[l] * B.nb[l] * B.groups[l];
  }
  for (int l = c.num_levels; l <= CN_CELL_LEVELS; ++l) B.first_block[l] = blocks;
  for (int l = c.num_levels; l < CN_CELL_LEVELS; ++l) B.nb[l] = B.groups[l] = 1;
  hipLaunchKernelGGL(cell_scatter_fold_blocks_kernel, dim3(blocks), dim3(256), 0, stream, B, gtab);
#endif
}

// fold the private copies into the gradient table and zero them again: 64 vertices of the dense n1^3 array per workgroup,
// the copies shared out over its 4 waves (each load is 64 consecutive float2 of one copy)
__global__ void __launch_bounds__(256) coarse_scatter_reduce_kernel(CoarseScatter c, Lvl lv, float* __restrict__ gtab) {
  __shared__ float2 part[4][64];
  const unsigned nv = c.n1 * c.n1 * c.n1;
  const unsigned j = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const unsigned v = blockIdx.x * 64u + j;
  float s0 = 0.f, s1 = 0.f;
  if (v < nv) {
    for (unsigned k = w; k < c.copies; k += 4) {
      float2* p = reinterpret_cast<float2*>(c.base) + (size_t)k * nv + v;
      const float2 t = *p;
      if (t.x != 0.f || t.y != 0.f) {
        s0 += t.x;
        s1 += t.y;
        *p = make_float2(0.f, 0.f);
      }
    }
  }
  part[w][j] = make_float2(s0, s1);
  __syncthreads();
  if (w != 0 || v >= nv) return;
  s0 = part[0][j].x + part[1][j].x + part[2][j].x + part[3][j].x;
  s1 = part[0][j].y + part[1][j].y + part[2][j].y + part[3][j].y;
  if (s0 == 0.f && s1 == 0.f) return;
  const unsigned x = v % c.n1, y = (v / c.n1) % c.n1, z = v / (c.n1 * c.n1);
  const unsigned e = ((x ^ (y * lv.m1) ^ (z * lv.m2)) & lv.mask) + lv.off;
  cn_atomic_add(gtab + 2 * (size_t)e, s0);
  cn_atomic_add(gtab + 2 * (size_t)e + 1, s1);
}
inline void launch_coarse_reduce(const CoarseScatter& c, const GridDev& grid, float* gtab, hipStream_t stream) {
  if (!c.base) return;
  const unsigned nv = c.n1 * c.n1 * c.n1;
  hipLaunchKernelGGL(coarse_scatter_reduce_kernel, dim3((nv + 63) / 64), dim3(256), 0, stream, c, grid.level(0), gtab);
}

// cells-per-sample ratio up to which a level's gradient goes through cell-major records:
// CN_CELL_SCATTER sets it for every backward kernel (0 = off).
static double cell_scatter_ratio(double dflt) {
  const char* cs = getenv("CN_CELL_SCATTER");
  return cs ? atof(cs) : dflt;
}

// ---- host side: what an entry point does before and after its backward kernel ----------------------------------------------
// The scratch a backward call over `samples` samples uses, into the CoarseScatter / CellScatter pair of the kernel's arguments:
// level 0's private copies, or -- where `cells_allowed` and the ratio (CN_CELL_SCATTER, else `default_ratio`; 0: off) admit any
// -- cell-major records for the levels with at most ratio x samples cells; level 0 is cell-major then and its private copies
// are off.  `samples_f` is the sample count as the entry multiplies it with the ratio, for an entry that forms it in floating
// point.
inline void plan_grid_scatter(const cn_grid& grads_grid, unsigned long long samples, double default_ratio, bool cells_allowed,
                              CoarseScatter& coarse, CellScatter& cells, double samples_f = -1.0) {
  coarse = make_coarse_scatter(grads_grid);
  cells = CellScatter{};
  const double ratio = cell_scatter_ratio(default_ratio);
  if (ratio != 0.0 && cells_allowed) {
    const unsigned long long max_cells = (unsigned long long)(samples_f >= 0.0 ? samples_f * ratio : samples * ratio);
    cells = make_cell_scatter(grads_grid, max_cells, samples);
  }
  if (cells.num_levels > 0) coarse.base = nullptr;
}

// Behind the backward kernel: fold the scratch into the gradient table and report launch errors under the entry's name.
// (Deterministic test build: the flushes turn the shadows into floats before the folds read them, and after.)
inline int finish_grid_scatter(const CoarseScatter& coarse, const CellScatter& cells, const GridDev& grid, float* gtab,
                               hipStream_t stream, const char* entry) {
  CN_DET_FLUSH(stream);
  launch_coarse_reduce(coarse, grid, gtab, stream);
  launch_cell_fold(cells, grid, gtab, stream);
  if (int rc = check_launch(entry)) return rc;
  CN_DET_FLUSH(stream);
  return CN_OK;
}

}  // namespace cn
