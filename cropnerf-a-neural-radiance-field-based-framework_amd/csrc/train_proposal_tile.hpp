// cn_proposal_backward, first form: four waves share a 64-sample tile, levels dealt out over the waves, activations in LDS.
// Launched under CN_PROP_BWD=tile only (A/B runs, cross-checks); the default is train_proposal_wave.hpp.
#pragma once

#include "train_field_scalar.hpp"  // fwd_rows, bwd_rows, WGrad, bias_add; the unit's shared header

namespace cn {

template <int L>
__global__ void __launch_bounds__(TB, 4) proposal_backward_kernel(PropBwdArgs A) {
  constexpr int K = 2 * L, H = 16;
  __shared__ float lds[(K + H + H + 1 + 4 + 3 + 12) * LD + 4 * 64 * 17];
  float* enc = lds;                  // [K]
  float* hid = enc + K * LD;         // [H] post ReLU
  float* dh = hid + H * LD;          // [H] delta hidden
  float* dout = dh + H * LD;         // [1] delta logit
  float* misc = dout + LD;           // normalised pos(3) sel(1) world pos(3) per-wave d(pos)(12)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform -> weights come through s_load
  float* tb = misc + 19 * LD + wave * (64 * 17);  // this wave's transpose buffer of hash_level_backward_cells
  WGrad<K, H> gW0;
  WGrad<H, 1> gW1;
  gW0.zero();
  gW1.zero();
  float gb0 = 0.f, gb1 = 0.f;
  const long long total = A.R * (long long)A.S;
  const long long ntiles = (total + TS - 1) / TS;
  // (one contiguous run of tiles per workgroup: train_field_mfma.hpp on batches sorted by camera and pixel)
  const long long tiles_per_wg = (ntiles + gridDim.x - 1) / gridDim.x;
  const long long tile_end = ((long long)blockIdx.x + 1) * tiles_per_wg < ntiles ? ((long long)blockIdx.x + 1) * tiles_per_wg : ntiles;
  for (long long tile = blockIdx.x * tiles_per_wg; tile < tile_end; ++tile) {
    const long long i = tile * TS + lane;
    const bool valid = i < total;
    const long long ic = valid ? i : total - 1;
    const long long r = ic / A.S;
    float sel_f = 0.f;
    if (wave == 0) {
      const float mid = (A.starts[ic] + A.ends[ic]) / 2.f;
      float px = A.origins[3 * r] + A.directions[3 * r] * mid;
      float py = A.origins[3 * r + 1] + A.directions[3 * r + 1] * mid;
      float pz = A.origins[3 * r + 2] + A.directions[3 * r + 2] * mid;
      misc[4 * LD + lane] = px;
      misc[5 * LD + lane] = py;
      misc[6 * LD + lane] = pz;
      bool sel = normalize_position(A.scene, px, py, pz);
      sel_f = sel ? 1.f : 0.f;
      misc[0 * LD + lane] = px;
      misc[1 * LD + lane] = py;
      misc[2 * LD + lane] = pz;
      misc[3 * LD + lane] = sel_f;
    }
    __syncthreads();
    // (levels shared out as in the scatter below, so that the Jacobian of a level's features with respect to the position --
    //  hash_level_jac: the position gradient without a second gather -- stays in the registers of the wave that needs it)
    v2f_t jx[2], jy[2], jz[2];
#pragma unroll
    for (int round = 0; round < 2; ++round) {
      const int l = round == 0 ? L - 1 - wave : L - 8 + wave;
      jx[round] = jy[round] = jz[round] = v2f_t{0.f, 0.f};
      if (l < 0) continue;
      float2 f = hash_level_jac(A.table, A.grid.level(l), A.grid.pos_offset, misc[lane], misc[LD + lane],
                                misc[2 * LD + lane], jx[round], jy[round], jz[round]);
      enc[(2 * l) * LD + lane] = f.x;
      enc[(2 * l + 1) * LD + lane] = f.y;
    }
    __syncthreads();
    fwd_rows<K, H, true>(A.w0, A.b0, enc, hid, wave, lane);
    __syncthreads();
    if (wave == 0) {
      float logit = A.b1[0];
#pragma unroll
      for (int k = 0; k < H; ++k) logit = fmaf(A.w1[k], hid[k * LD + lane], logit);
      const float up = valid ? A.d_density[ic] : 0.f;
      dout[lane] = up * misc[3 * LD + lane] * expf(fminf(fmaxf(logit, -15.f), 15.f));
    }
    __syncthreads();
    gW1.add(dout, hid, tid);
    bias_add<1>(gb1, dout, tid);
    bwd_rows<H, 1>(A.w1, dout, dh, hid, 0, H, wave, lane);
    __syncthreads();
    gW0.add(dh, enc, tid);
    bias_add<H>(gb0, dh, tid);
    // delta_enc[k] = sum_n W0[n][k] dh[n] -> straight into the table gradient
    float gpx = 0.f, gpy = 0.f, gpz = 0.f;
    // the finest level costs most (one request per x-edge, no runs to merge) and the coarsest least: the waves take the
    // levels from the fine end, the second round from the other side (L = 5: {4}, {3}, {2}, {1, 0})
#pragma unroll
    for (int round = 0; round < 2; ++round) {
      const int l = round == 0 ? L - 1 - wave : L - 8 + wave;
      if (l < 0) continue;
      float g0 = 0.f, g1 = 0.f;
#pragma unroll
      for (int n = 0; n < H; ++n) {
        const float d = dh[n * LD + lane];
        g0 = fmaf(A.w0[n * K + 2 * l], d, g0);
        g1 = fmaf(A.w0[n * K + 2 * l + 1], d, g1);
      }
      g0 = valid ? g0 : 0.f;
      g1 = valid ? g1 : 0.f;
      gpx += g0 * jx[round].x + g1 * jx[round].y;
      gpy += g0 * jy[round].x + g1 * jy[round].y;
      gpz += g0 * jz[round].x + g1 * jz[round].y;
      float ux = 0.f, uy = 0.f, uz = 0.f;  // (unused: the <false> forms do not touch them)
      if (l < A.cells.num_levels) {
        const unsigned nl = A.cells.n[l];
        float* rec = A.cells.base + A.cells.offset[l] +
                     (size_t)(blockIdx.x % A.cells.copies[l]) * ((size_t)nl * nl * nl * 16);
        hash_level_backward_cells<false>(rec, nl, tb, A.g_table, A.table, A.grid.level(l), A.grid.pos_offset, misc[lane],
                                         misc[LD + lane], misc[2 * LD + lane], g0, g1, lane, ux, uy, uz);
      } else if (l == 0 && A.coarse.base) {
        float* mine = A.coarse.base + (size_t)(blockIdx.x % A.coarse.copies) * (2u * A.coarse.n1 * A.coarse.n1 * A.coarse.n1);
        hash_level_backward_private<false>(mine, A.coarse.n1, A.g_table, A.table, A.grid.level(0), A.grid.pos_offset,
                                           misc[lane], misc[LD + lane], misc[2 * LD + lane], g0, g1, lane, ux, uy, uz);
      } else
        hash_level_backward<false>(A.g_table, A.table, A.grid.level(l), A.grid.pos_offset, misc[lane],
                                   misc[LD + lane], misc[2 * LD + lane], g0, g1, lane, ux, uy, uz);
    }
    if (A.d_pos) {
      misc[(7 + 3 * wave) * LD + lane] = gpx;
      misc[(8 + 3 * wave) * LD + lane] = gpy;
      misc[(9 + 3 * wave) * LD + lane] = gpz;
      __syncthreads();
      if (wave == 0 && valid) {
        float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          gx += misc[(7 + 3 * w) * LD + lane];
          gy += misc[(8 + 3 * w) * LD + lane];
          gz += misc[(9 + 3 * w) * LD + lane];
        }
        normalize_position_backward(A.scene, misc[4 * LD + lane], misc[5 * LD + lane], misc[6 * LD + lane],
                                    misc[3 * LD + lane], gx, gy, gz);
        A.d_pos[3 * i] = gx;
        A.d_pos[3 * i + 1] = gy;
        A.d_pos[3 * i + 2] = gz;
      }
    }
    __syncthreads();
  }
  gW0.flush(A.g_w0, tid);
  gW1.flush(A.g_w1, tid);
  if (tid < H) cn_atomic_add(A.g_b0 + tid, gb0);
  if (tid < 1) cn_atomic_add(A.g_b1 + tid, gb1);
}

}  // namespace cn
