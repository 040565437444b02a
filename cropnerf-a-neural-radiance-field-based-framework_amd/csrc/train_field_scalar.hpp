// The first FruitField backward kernel, on scalar FMAs: cn_field_backward launches it under CN_FIELD_BACKWARD_IMPL=scalar only
// (the default is train_field_mfma.hpp).  Kept as an independent device implementation for cross-checks.
//
// Layout: a 256-thread workgroup owns a tile of 64 samples; activations and deltas live in LDS as [feature][65]
// (row pad 1 -> conflict-free both for "lane = sample" sweeps and for the weight-gradient dots).  Forward / delta
// layers split their output rows over the 4 waves (weights come through scalar loads).  Weight gradients
// dW[n][k] = sum_samples delta[n] x[k]: thread t owns entries t, t+256, ... of each matrix and keeps the partial sums in
// registers across all tiles of its (persistent) workgroup, then issues one global_atomic_add_f32 per entry at the end
// -- atomics per step are (#workgroups x #parameters), not (#samples x #parameters).  Every level takes the table path of
// the scatter (hash_level_backward).  The row helpers below also serve the tile form of the proposal backward
// (train_proposal_tile.hpp).
#pragma once

#include "train_field_common.hpp"

namespace cn {

// y[n][lane] = act(b[n] + sum_k W[n][k] x[k][lane]) for the rows n = wave, wave+4, ...
template <int K, int N, bool RELU>
__device__ __forceinline__ void fwd_rows(const float* __restrict__ Wg, const float* __restrict__ bg, const float* x,
                                         float* y, int wave, int lane) {
  const cfloat_ptr W = as_const(Wg), b = as_const(bg);
  for (int n = wave; n < N; n += 4) {
    float acc = b[n];
#pragma unroll 8
    for (int k = 0; k < K; ++k) acc = fmaf(W[n * K + k], x[k * LD + lane], acc);
    y[n * LD + lane] = RELU ? fmaxf(acc, 0.f) : acc;
  }
}

// dx[k][lane] = (sum_n W[n][k] dy[n][lane]) * (gate ? act[k][lane] > 0 : 1) for rows k = k0 + wave, +4, ... < k1
template <int K, int N>
__device__ __forceinline__ void bwd_rows(const float* __restrict__ Wg, const float* dy, float* dx, const float* act,
                                         int k0, int k1, int wave, int lane) {
  const cfloat_ptr W = as_const(Wg);
  for (int k = k0 + wave; k < k1; k += 4) {
    float acc = 0.f;
#pragma unroll 8
    for (int n = 0; n < N; ++n) acc = fmaf(W[n * K + k], dy[n * LD + lane], acc);
    if (act) acc = act[k * LD + lane] > 0.f ? acc : 0.f;
    dx[k * LD + lane] = acc;
  }
}

// acc[i] += sum_j dy[n][j] x[k][j] for the entries e = tid + TB*i (n = e / K, k = e % K)
template <int K, int N>
struct WGrad {
  static constexpr int E = (N * K + TB - 1) / TB;
  float acc[E];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < E; ++i) acc[i] = 0.f;
  }
  __device__ __forceinline__ void add(const float* dy, const float* x, int tid) {
#pragma unroll
    for (int i = 0; i < E; ++i) {
      int e = tid + TB * i;
      if (e < N * K) {
        const float* a = dy + (e / K) * LD;
        const float* b = x + (e % K) * LD;
        float s = 0.f;
#pragma unroll 8
        for (int j = 0; j < TS; ++j) s = fmaf(a[j], b[j], s);
        acc[i] += s;
      }
    }
  }
  __device__ __forceinline__ void flush(float* __restrict__ g, int tid) {
#pragma unroll
    for (int i = 0; i < E; ++i) {
      int e = tid + TB * i;
      if (e < N * K) cn_atomic_add(g + e, acc[i]);
    }
  }
};

// bias gradient: thread n < N owns sum_j dy[n][j]
template <int N>
__device__ __forceinline__ void bias_add(float& acc, const float* dy, int tid) {
  if (tid < N) {
    float s = 0.f;
#pragma unroll 8
    for (int j = 0; j < TS; ++j) s += dy[tid * LD + j];
    acc += s;
  }
}

// LDS rows (each LD floats)
constexpr int R_ENC = 0;            // 32
constexpr int R_H1 = R_ENC + 32;    // 64 (post ReLU)
constexpr int R_O16 = R_H1 + 64;    // 16
constexpr int R_S1 = R_O16 + 16;    // 64 (post ReLU)
constexpr int R_S2 = R_S1 + 64;     // 64
constexpr int R_CIN = R_S2 + 64;    // 63 (+1 pad row)
constexpr int R_C1 = R_CIN + 64;    // 64
constexpr int R_C2 = R_C1 + 64;     // 64
constexpr int R_DA = R_C2 + 64;     // 64 delta buffer A
constexpr int R_DB = R_DA + 64;     // 64 delta buffer B
// misc rows: 0-2 normalised position, 3 selector, 4 d(logit), 5 d(sem), 6-8 world position, 9-20 per-wave partial
// d(loss)/d(normalised position) (3 per wave)
constexpr int R_MISC = R_DB + 64;
constexpr int FIELD_ROWS = R_MISC + 21;

__global__ void __launch_bounds__(TB) field_backward_kernel(FieldBwdArgs A) {
  extern __shared__ __align__(16) float lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform -> weights come through s_load
  float* enc = lds + R_ENC * LD;
  float* h1 = lds + R_H1 * LD;
  float* o16 = lds + R_O16 * LD;
  float* s1 = lds + R_S1 * LD;
  float* s2 = lds + R_S2 * LD;
  float* cin = lds + R_CIN * LD;
  float* c1 = lds + R_C1 * LD;
  float* c2 = lds + R_C2 * LD;
  float* dA = lds + R_DA * LD;
  float* dB = lds + R_DB * LD;
  float* misc = lds + R_MISC * LD;

  WGrad<32, 64> gW0;
  WGrad<64, 16> gW1;
  WGrad<15, 64> gWs0;
  WGrad<64, 64> gWs1;
  WGrad<63, 64> gWc0;
  WGrad<64, 64> gWc1;
  WGrad<64, 3> gWc2;
  WGrad<64, 1> gWh;
  gW0.zero(); gW1.zero(); gWs0.zero(); gWs1.zero(); gWc0.zero(); gWc1.zero(); gWc2.zero(); gWh.zero();
  float gb0 = 0.f, gb1 = 0.f, gbs0 = 0.f, gbs1 = 0.f, gbh = 0.f, gbc0 = 0.f, gbc1 = 0.f, gbc2 = 0.f;

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
    // ---- per-sample inputs (wave 0 fills the shared rows) ------------------------------------------------------
    if (wave == 0) {
      const float mid = (A.starts[ic] + A.ends[ic]) / 2.f;
      float px = A.origins[3 * r] + A.directions[3 * r] * mid;
      float py = A.origins[3 * r + 1] + A.directions[3 * r + 1] * mid;
      float pz = A.origins[3 * r + 2] + A.directions[3 * r + 2] * mid;
      misc[6 * LD + lane] = px;
      misc[7 * LD + lane] = py;
      misc[8 * LD + lane] = pz;
      bool sel = normalize_position(A.scene, px, py, pz);
      misc[0 * LD + lane] = px;
      misc[1 * LD + lane] = py;
      misc[2 * LD + lane] = pz;
      misc[3 * LD + lane] = sel ? 1.f : 0.f;
      misc[5 * LD + lane] = valid ? A.d_sem[ic] : 0.f;
      // colour input: SH(16) | geo (filled after the base MLP) | appearance(32)
      float dx = A.directions[3 * r], dy = A.directions[3 * r + 1], dz = A.directions[3 * r + 2];
      if (!A.sh_unit) {
        dx = (dx + 1.f) / 2.f;
        dy = (dy + 1.f) / 2.f;
        dz = (dz + 1.f) / 2.f;
      }
      float sh[16];
      sh_deg4(dx, dy, dz, sh);
#pragma unroll
      for (int k = 0; k < 16; ++k) cin[k * LD + lane] = sh[k];
      const float* a = A.app_per_camera ? A.p.emb + A.cam_idx[r] * 32 : A.app_mean;
      for (int k = 0; k < 32; ++k) cin[(31 + k) * LD + lane] = a ? a[k] : 0.f;
    }
    __syncthreads();
    // ---- forward recompute -------------------------------------------------------------------------------------------
    {
      const float px = misc[0 * LD + lane], py = misc[1 * LD + lane], pz = misc[2 * LD + lane];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int l = 4 * wave + q;
        float2 f = hash_level(A.p.table, A.grid.level(l), A.grid.pos_offset, px, py, pz);
        enc[(2 * l) * LD + lane] = f.x;
        enc[(2 * l + 1) * LD + lane] = f.y;
      }
    }
    __syncthreads();
    fwd_rows<32, 64, true>(A.p.w0, A.p.b0, enc, h1, wave, lane);
    __syncthreads();
    fwd_rows<64, 16, false>(A.p.w1, A.p.b1, h1, o16, wave, lane);
    __syncthreads();
    if (wave == 0) {
      // trunc_exp backward: g * exp(clamp(x, -15, 15)), times the selector; d_density is d loss / d (post-selector density)
      const float logit = o16[lane];
      const float dd = valid ? A.d_density[ic] : 0.f;
      misc[4 * LD + lane] = dd * misc[3 * LD + lane] * expf(fminf(fmaxf(logit, -15.f), 15.f));
    }
    for (int k = wave; k < 15; k += 4) cin[(16 + k) * LD + lane] = o16[(1 + k) * LD + lane];
    fwd_rows<15, 64, true>(A.p.ws0, A.p.bs0, o16 + LD, s1, wave, lane);  // geo = rows 1..15 of o16
    __syncthreads();
    fwd_rows<64, 64, false>(A.p.ws1, A.p.bs1, s1, s2, wave, lane);
    fwd_rows<63, 64, true>(A.p.wc0, A.p.bc0, cin, c1, wave, lane);
    __syncthreads();
    fwd_rows<64, 64, true>(A.p.wc1, A.p.bc1, c1, c2, wave, lane);
    __syncthreads();
    // ---- colour head: rgb = sigmoid(Wc2 c2 + bc2); delta_pre = d_rgb * rgb (1 - rgb) -> dA rows 0..2 ----------------
    if (wave < 3) {
      float acc = A.p.bc2[wave];
      for (int k = 0; k < 64; ++k) acc = fmaf(A.p.wc2[wave * 64 + k], c2[k * LD + lane], acc);
      const float s = 1.f / (1.f + expf(-acc));
      const float up = valid ? A.d_rgb[3 * ic + wave] : 0.f;
      dA[wave * LD + lane] = up * s * (1.f - s);
    }
    __syncthreads();
    gWc2.add(dA, c2, tid);
    bias_add<3>(gbc2, dA, tid);
    bwd_rows<64, 3>(A.p.wc2, dA, dB, c2, 0, 64, wave, lane);  // delta_c2 (ReLU-gated) -> dB
    __syncthreads();
    gWc1.add(dB, c1, tid);
    bias_add<64>(gbc1, dB, tid);
    bwd_rows<64, 64>(A.p.wc1, dB, dA, c1, 0, 64, wave, lane);  // delta_c1 -> dA
    __syncthreads();
    gWc0.add(dA, cin, tid);
    bias_add<64>(gbc0, dA, tid);
    // delta of the colour input: geo rows (16..30) feed the base MLP, appearance rows (31..62) the embedding
    // (rows 0..15, the SH inputs, only when the direction gradient is wanted)
    bwd_rows<63, 64>(A.p.wc0, dA, dB, nullptr, A.d_dir ? 0 : 16, 63, wave, lane);  // dB rows 16..62
    __syncthreads();
    if (A.app_per_camera && valid) {
      for (int k = wave; k < 32; k += 4) cn_atomic_add(A.g.emb + A.cam_idx[r] * 32 + k, dB[(31 + k) * LD + lane]);
    }
    if (A.d_dir && wave == 3 && valid) {
      float gsh[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) gsh[k] = dB[k * LD + lane];
      float dx = A.directions[3 * r], dy = A.directions[3 * r + 1], dz = A.directions[3 * r + 2];
      const float chain = A.sh_unit ? 1.f : 0.5f;
      if (!A.sh_unit) {
        dx = (dx + 1.f) / 2.f;
        dy = (dy + 1.f) / 2.f;
        dz = (dz + 1.f) / 2.f;
      }
      float gx, gy, gz;
      sh_deg4_backward(dx, dy, dz, gsh, gx, gy, gz);
      A.d_dir[3 * i] = gx * chain;
      A.d_dir[3 * i + 1] = gy * chain;
      A.d_dir[3 * i + 2] = gz * chain;
    }
    // delta_o16 -> dA' : row 0 = density logit, rows 1..15 = geo (from the colour branch only: semantics sees detached geo)
    // (dA is still needed by nobody: gWc0 has consumed it)
    __syncthreads();
    if (wave == 0) dA[lane] = misc[4 * LD + lane];
    for (int k = wave; k < 15; k += 4) dA[(1 + k) * LD + lane] = dB[(16 + k) * LD + lane];
    __syncthreads();
    gW1.add(dA, h1, tid);
    bias_add<16>(gb1, dA, tid);
    bwd_rows<64, 16>(A.p.w1, dA, dB, h1, 0, 64, wave, lane);  // delta_h1 -> dB
    __syncthreads();
    gW0.add(dB, enc, tid);
    bias_add<64>(gb0, dB, tid);
    bwd_rows<32, 64>(A.p.w0, dB, dA, nullptr, 0, 32, wave, lane);  // delta_enc -> dA rows 0..31
    __syncthreads();
    const float px = misc[0 * LD + lane], py = misc[1 * LD + lane], pz = misc[2 * LD + lane];
    float gpx = 0.f, gpy = 0.f, gpz = 0.f;
    if (A.d_pos) {  // kernel-uniform
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int l = 4 * wave + q;
        hash_level_backward<true>(A.g.table, A.p.table, A.grid.level(l), A.grid.pos_offset, px, py, pz,
                                  valid ? dA[(2 * l) * LD + lane] : 0.f, valid ? dA[(2 * l + 1) * LD + lane] : 0.f,
                                  lane, gpx, gpy, gpz);
      }
      misc[(9 + 3 * wave) * LD + lane] = gpx;
      misc[(10 + 3 * wave) * LD + lane] = gpy;
      misc[(11 + 3 * wave) * LD + lane] = gpz;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int l = 4 * wave + q;
        hash_level_backward<false>(A.g.table, A.p.table, A.grid.level(l), A.grid.pos_offset, px, py, pz,
                                   valid ? dA[(2 * l) * LD + lane] : 0.f, valid ? dA[(2 * l + 1) * LD + lane] : 0.f,
                                   lane, gpx, gpy, gpz);
      }
    }
    __syncthreads();
    if (A.d_pos && wave == 3 && valid) {
      float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        gx += misc[(9 + 3 * w) * LD + lane];
        gy += misc[(10 + 3 * w) * LD + lane];
        gz += misc[(11 + 3 * w) * LD + lane];
      }
      normalize_position_backward(A.scene, misc[6 * LD + lane], misc[7 * LD + lane], misc[8 * LD + lane],
                                  misc[3 * LD + lane], gx, gy, gz);
      A.d_pos[3 * i] = gx;
      A.d_pos[3 * i + 1] = gy;
      A.d_pos[3 * i + 2] = gz;
    }
    // ---- semantic branch: sem = Wh s2 + bh; gradients stop at the (detached) geo features ------------------------------
    // delta_sem (1 row) is misc row 5
    gWh.add(misc + 5 * LD, s2, tid);
    bias_add<1>(gbh, misc + 5 * LD, tid);
    bwd_rows<64, 1>(A.p.wh, misc + 5 * LD, dB, nullptr, 0, 64, wave, lane);  // delta_s2 -> dB
    __syncthreads();
    gWs1.add(dB, s1, tid);
    bias_add<64>(gbs1, dB, tid);
    bwd_rows<64, 64>(A.p.ws1, dB, dA, s1, 0, 64, wave, lane);  // delta_s1 -> dA
    __syncthreads();
    gWs0.add(dA, o16 + LD, tid);
    bias_add<64>(gbs0, dA, tid);
    __syncthreads();
  }
  gW0.flush(A.g.w0, tid); gW1.flush(A.g.w1, tid); gWs0.flush(A.g.ws0, tid); gWs1.flush(A.g.ws1, tid);
  gWc0.flush(A.g.wc0, tid); gWc1.flush(A.g.wc1, tid); gWc2.flush(A.g.wc2, tid); gWh.flush(A.g.wh, tid);
  if (tid < 64) {
    cn_atomic_add(A.g.b0 + tid, gb0);
    cn_atomic_add(A.g.bs0 + tid, gbs0);
    cn_atomic_add(A.g.bs1 + tid, gbs1);
    cn_atomic_add(A.g.bc0 + tid, gbc0);
    cn_atomic_add(A.g.bc1 + tid, gbc1);
  }
  if (tid < 16) cn_atomic_add(A.g.b1 + tid, gb1);
  if (tid < 3) cn_atomic_add(A.g.bc2 + tid, gbc2);
  if (tid < 1) cn_atomic_add(A.g.bh + tid, gbh);
}

}  // namespace cn
