// render_f16_kernel -- the DENSITY-ONLY pass of the fp16 matrix mode (cn_render_opts.matrix_precision = CN_MATRIX_F16 with
// density_only: get_density_for_camera_ray_bundle, the occlusion pass of the projection), for which render_split_kernel has
// no variant; the composited and per-sample fp16 renders run render_split_kernel<., MM_F16, ., .>.  The fp16 mode is the
// reference's OWN arithmetic class: tiny-cuda-nn's FullyFusedMLP under mixed precision (fruit_nerf/fruit_field.py:95,125-167
// build every module with implementation="tcnn"; fruit_nerf_config.py:35 mixed_precision=True).  Included by render_fused.hip.
//
// Every wave owns a ray end to end (28.8 KB LDS image: five 4-wave workgroups fit a CU).  The kernel was first built as THE
// fp16 renderer, colour and per-sample outputs included, on the reasoning that with fp16 operands the kernel is its hash-grid
// gathers and independent waves hide their latency better than the producer/consumer kernel's lock-step.  It lost (C2 on a
// tcnn fp16 table: 2.9 against 1.6 ms): what the gathers cost is L1 line lookups and misses, and the split
// kernel's eight rays -- neighbouring pixels at the same depth -- share their lines.  Its colour and per-sample forms, and
// the switch that selected them, were removed.
//
// Arithmetic (the parity bar is oracle/tcnn.py with tcnn_half_activations=True, tests/test_gpu_f16.py):
//   * weights rounded to fp16 in prep_kernel (a no-op for an imported tcnn checkpoint, whose parameters are fp16 values);
//   * half table: the trilinear blend runs on packed fp16 pairs (hash_level_pk_*: v_pk_fma_f16, 14 instructions for both
//     features, x-pair gathers), as tcnn's kernel_grid accumulates in the parameter type; float table: fp32 blend, result
//     rounded to fp16;
//   * every layer input rounded to fp16 (v_cvt_pk_f16_f32, round to nearest even), products summed in fp32 by the MFMA
//     (tcnn accumulates in fp16: this is at least as precise), biases and compositing in fp32.
// Ray -> wave scheduling (XCD column stripes), compositing and early termination are render_fused_kernel's.
#pragma once

namespace cn {

#ifndef CN_F16_WAVES_PER_SIMD
#define CN_F16_WAVES_PER_SIMD 4
#endif
#ifndef CN_F16_LEVELS_IN_FLIGHT
#define CN_F16_LEVELS_IN_FLIGHT 2
#endif

// LDS image of a workgroup: the 22 fp16 A-operand blocks, then the blob from OFF_B0 on (biases, folded heads, SH columns,
// level records) -- 28.8 KB instead of the 43 KB of the fp32 image, so that five 4-wave workgroups fit a CU.
constexpr int F16_IMG_FLOATS = BF16_BLOCKS * 256;
constexpr int F16_TAIL_FLOATS = BLOB_FLOATS - OFF_B0;
constexpr int F16_LDS_FLOATS = F16_IMG_FLOATS + F16_TAIL_FLOATS + FUSED_WAVES * WAVE_SCRATCH;
static_assert(F16_IMG_FLOATS % 4 == 0 && F16_TAIL_FLOATS % 4 == 0 && OFF_B0 % 4 == 0, "copied as float4");
#define CN_F16_T(OFF) (F16_IMG_FLOATS + (OFF) - OFF_B0)  // LDS float index of blob offset OFF (>= OFF_B0)

template <bool HALF, bool GENERIC>
__global__ void __launch_bounds__(FUSED_THREADS, CN_F16_WAVES_PER_SIMD) render_f16_kernel(FusedArgs A) {
  __shared__ __align__(16) float lds[F16_LDS_FLOATS];
  {
    const float4* src = reinterpret_cast<const float4*>(A.blob);
    float4* dst = reinterpret_cast<float4*>(lds);
    for (int i = threadIdx.x; i < F16_IMG_FLOATS / 4; i += FUSED_THREADS) dst[i] = src[i];
    for (int i = threadIdx.x; i < F16_TAIL_FLOATS / 4; i += FUSED_THREADS) dst[F16_IMG_FLOATS / 4 + i] = src[OFF_B0 / 4 + i];
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const int g = lane >> 4, j = lane & 15;
  float* tbuf = lds + F16_IMG_FLOATS + F16_TAIL_FLOATS + wave * WAVE_SCRATCH + 64;  // [0,65): bin edges
  const int S = A.S;
  auto blkh = [&](int b) { return reinterpret_cast<const f16x8*>(lds + b * 256)[lane]; };

  const int nchunks = (S + 63) >> 6;
  const int xcd = blockIdx.x & 7;
  const int slot = blockIdx.x >> 3;
  const long long stride = (long long)(gridDim.x >> 3) * FUSED_WAVES;
  const bool striped = A.image_width > 0;
  const long long per_xcd = (A.num_rays + 7) >> 3;
  const int nstripe = 8 * A.stripes_per_xcd;
  const int cw = striped ? (A.image_width + nstripe - 1) / nstripe : 0;
  const long long first_row = striped ? A.pixel_start / A.image_width : 0;
  const long long last_row = striped ? (A.pixel_start + A.num_rays - 1) / A.image_width : 0;
  const long long rows = last_row - first_row + 1;
  const long long items = striped ? rows * cw * A.stripes_per_xcd : min(per_xcd, max(A.num_rays - xcd * per_xcd, 0LL));

  for (long long q = slot * FUSED_WAVES + wave; q < items; q += stride) {
    long long rr;
    if (striped) {
      const long long sq = q / (rows * cw);
      const long long qq = q - sq * rows * cw;
      const long long vrow = qq / cw;
      const int col = (int)(sq * 8 + xcd) * cw + (int)(qq - vrow * cw);
      rr = (first_row + vrow) * A.image_width + col - A.pixel_start;
      if (col >= A.image_width || rr < 0 || rr >= A.num_rays) continue;  // wave-uniform
    } else {
      rr = xcd * per_xcd + q;
    }
    const long long r = __builtin_amdgcn_readfirstlane((int)rr);
    const float ox = A.origins[3 * r], oy = A.origins[3 * r + 1], oz = A.origins[3 * r + 2];
    const float dx = A.directions[3 * r], dy = A.directions[3 * r + 1], dz = A.directions[3 * r + 2];
    const float sn = spacing_fn(A.spacing, A.nears[r]), sf = spacing_fn(A.spacing, A.fars[r]);
    const float* bins = A.bins ? A.bins + r * (long long)(S + 1) : nullptr;
    auto edge = [&](int i) -> float {
      i = min(i, S);
      return bins ? bins[i] : spacing_to_euclid(A.spacing, linspace01(i, S + 1, A.lin_step), sn, sf);
    };

    CompositeState st;
    for (int ch = 0; ch < nchunks; ++ch) {
      const int c0 = ch * 64;
      const float e_lo = edge(c0 + lane);
      const float e_top = edge(c0 + 64);
      __builtin_amdgcn_wave_barrier();
      tbuf[lane] = e_lo;
      if (lane == 0) tbuf[64] = e_top;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();

      float my_dlogit = 0.f, my_sel = 0.f;
#pragma unroll 1
      for (int half = 0; half < 2; ++half) {
        float px[2], py[2], pz[2];
        bool sel[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int k = 32 * half + 16 * c + j;
          const float mid = (tbuf[k] + tbuf[k + 1]) / 2.f;
          px[c] = ox + dx * mid;
          py[c] = oy + dy * mid;
          pz[c] = oz + dz * mid;
          sel[c] = normalize_position(A.scene, px[c], py[c], pz[c]);
        }
        // ---- hash grid: levels 4g..4g+3 of the two samples, as the packed fp16 pairs the first MFMA consumes ----------
        u32x4v featp[2];
        {
          const f32x4 lvl_scale = *reinterpret_cast<const f32x4*>(lds + CN_F16_T(OFF_SCALE) + 4 * g);
          const float pos_off = GENERIC ? A.grid.pos_offset : 0.f;
          if constexpr (HALF && !CN_ABLATE_GATHER) {
            // pair gathers: the eight (level, sample) units in program order, unit n + 1's loads issued before unit n is blended
            PkLoads cur = hash_level_pk_issue<GENERIC>(
                A.grid.table, lane_level_rec<GENERIC>(lds + CN_F16_T(OFF_LVL), A.grid, 4 * g, lvl_scale[0]), pos_off, px[0], py[0], pz[0]);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              PkLoads nxt;
              if (u < 7) {
                const int qn = (u + 1) >> 1, cn_ = (u + 1) & 1;
                nxt = hash_level_pk_issue<GENERIC>(
                    A.grid.table, lane_level_rec<GENERIC>(lds + CN_F16_T(OFF_LVL), A.grid, 4 * g + qn, lvl_scale[qn]), pos_off, px[cn_],
                    py[cn_], pz[cn_]);
              }
              featp[u & 1][u >> 1] = pk_pin(hash_level_pk_blend(cur));
              if (u < 7) cur = nxt;
            }
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const Lvl lv = lane_level_rec<GENERIC>(lds + CN_F16_T(OFF_LVL), A.grid, 4 * g + q, lvl_scale[q]);
#pragma unroll
              for (int c = 0; c < 2; ++c) {
#if CN_ABLATE_GATHER  // timing-only build: no table reads
                featp[c][q] = __builtin_bit_cast(unsigned, px[c] * lv.scale + py[c]) ^ __builtin_bit_cast(unsigned, pz[c]);
#else
                const float2 f = hash_level_sc<HALF, GENERIC>(A.grid.table, lv, pos_off, px[c], py[c], pz[c]);
                const f16x2 hp = {(_Float16)f.x, (_Float16)f.y};
                featp[c][q] = __builtin_bit_cast(unsigned, hp);
#endif
              }
              if ((q + 1) % CN_F16_LEVELS_IN_FLIGHT == 0) __builtin_amdgcn_sched_barrier(0);
            }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- base MLP: 32 -> 64 ReLU -> 16 (neuron 0 = density logit, 1..15 = geo features) -----------------------------
        f16x8 hh[2][2];  // [K block][column tile]: the hidden layer as the next layer's B operands
        {
          f32x4 h[4][2];
#pragma unroll
          for (int mt = 0; mt < 4; ++mt) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(lds + CN_F16_T(OFF_B0) + 16 * mt + 4 * g);
            const f16x8 a = blkh(mt);
#pragma unroll
            for (int c = 0; c < 2; ++c) h[mt][c] = relu4(mfma_f16(a, __builtin_bit_cast(f16x8, featp[c]), b));
          }
#pragma unroll
          for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int c = 0; c < 2; ++c) hh[kb][c] = cvt_f16x8(h[2 * kb][c], h[2 * kb + 1][c]);
        }
        f32x4 o16[2];
        {
          const f32x4 b1 = *reinterpret_cast<const f32x4*>(lds + CN_F16_T(OFF_B1) + 4 * g);
          o16[0] = b1;
          o16[1] = b1;
#pragma unroll
          for (int kb = 0; kb < 2; ++kb) {
            const f16x8 a = blkh(4 + kb);
#pragma unroll
            for (int c = 0; c < 2; ++c) o16[c] = mfma_f16(a, hh[kb][c], o16[c]);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        const bool mine = (g >> 1) == half;  // this half holds lane l's own sample in column tile g & 1
        const bool odd = (g & 1) != 0;
        {
          const float d0 = row0_broadcast(o16[0].x), d1 = row0_broadcast(o16[1].x);
          my_dlogit = mine ? (odd ? d1 : d0) : my_dlogit;
          my_sel = mine ? ((odd ? sel[1] : sel[0]) ? 1.f : 0.f) : my_sel;
        }
      }
      // ---- lane l now holds sample c0 + l -----------------------------------------------------------------------------------
      const float density = expf(my_dlogit) * my_sel;
      const float sem = 0.f, cr = 0.f, cg = 0.f, cb = 0.f;  // (density only: the compositing's colour and semantics are zero)
      const int i = c0 + lane;
      const bool valid = i < S;
      const float e0 = e_lo, e1 = tbuf[lane + 1];
      const float mid = (e0 + e1) / 2.f;
      const float w = composite_chunk(st, valid, i == S - 1, e1 - e0, density, mid, cr, cg, cb, sem, A.eval_clamp != 0);
      if (A.out_w && valid) A.out_w[r * (long long)S + i] = w;
      // optional early ray termination, as render_fused_kernel (off by default)
      if (A.early_stop > 0.f && c0 + 64 < S && __expf(-st.carry_dd) < A.early_stop) {  // wave-uniform
        st.last_r = wave_read(A.eval_clamp ? nan_to_num(cr) : cr, 63);
        st.last_g = wave_read(A.eval_clamp ? nan_to_num(cg) : cg, 63);
        st.last_b = wave_read(A.eval_clamp ? nan_to_num(cb) : cb, 63);
        st.last_mid = wave_read(mid, 63);
        if (A.out_w)
          for (int k = c0 + 64 + lane; k < S; k += 64) A.out_w[r * (long long)S + k] = 0.f;
        break;
      }
    }
    const CompositeOut o = composite_finish(st, A.bg_mode, A.bg[0], A.bg[1], A.bg[2], A.eval_clamp != 0);
    if (lane == 0) {
      if (A.out_acc) A.out_acc[r] = o.acc;
      if (A.out_depth) A.out_depth[r] = o.depth;
    }
  }
}

}  // namespace cn
