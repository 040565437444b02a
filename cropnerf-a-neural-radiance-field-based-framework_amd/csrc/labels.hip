// labels.hip -- colour instance masks -> 8-bit label frames on the device (the reference's
// fruit_nerf/utils/convert_segmentation_img_to_label.py, step 1 of its workflow; the frames feed the merger's image stage,
// contour.hip).  A batch of F RGB frames [F,H,W,3] that are already in HBM goes through three launches.
//
// Definition (exact, see include/cropnerf_hip.h): key = B << 16 | G << 8 | R; black -> 0; any other pixel ->
// 1 + the number of distinct non-zero keys of ITS frame that are smaller.  The reference numbers the colours in the
// iteration order of a Python set, an arbitrary bijection onto 1..n; its consumers compare labels for equality within a
// frame and against 0 only, so the sorted order taken here is one of the labelings it can produce.
//
// Decomposition:
//   collect  every workgroup gathers the distinct keys of its pixels in an open-addressing set in LDS (a thread skips a
//            key equal to its previous one: neighbouring pixels mostly repeat), then merges the set into the frame's table
//            in the workspace;
//   rank     one workgroup per frame compacts the table, counts for every key the smaller ones and writes colors[] and
//            num_colors[];
//   apply    every workgroup rebuilds key -> label from colors[] in LDS and labels its pixels.
// Every probe sequence is at most LBL_SLOTS steps long and ends in the frame's overflow flag; no thread waits for
// another; labels are ranks of key VALUES, so nothing depends on the order in which waves insert.  A frame starts at byte
// f * H * W * 3, which need not be dword aligned: the up to three pixels before the first aligned 12-byte group and the up
// to three after the last whole group go through byte loads, everything between as four pixels = three dwords per thread.
#include "cn_common.hpp"

namespace cn {

constexpr int LBL_SLOTS = 1024;  // slots of a set (a power of two, four times the 255 keys of a valid frame)
constexpr int LBL_HDR = 16;      // words behind a frame's table in the workspace; [0] = overflow flag
constexpr unsigned LBL_MAX = 255;

__device__ __forceinline__ unsigned lbl_hash(unsigned key) { return (key * 2654435761u) >> 22; }  // 10 bits

struct LblSpan {  // one frame's pixels: [0, head) bytewise, `groups` aligned groups of four, then `tail` bytewise
  const uint8_t* px;
  int head, tail;
  long long groups;
};
__device__ __forceinline__ LblSpan lbl_span(const uint8_t* frames, long long f, long long hw) {
  LblSpan s;
  s.px = frames + f * hw * 3;
  // address + 3 p = 0 (mod 4)  <=>  p = address (mod 4)
  const long long head = (long long)(reinterpret_cast<uintptr_t>(s.px) & 3);
  s.head = (int)(head < hw ? head : hw);
  s.groups = (hw - s.head) / 4;
  s.tail = (int)(hw - s.head - 4 * s.groups);
  return s;
}
__device__ __forceinline__ unsigned lbl_key_at(const uint8_t* px, long long p) {
  return (unsigned)px[3 * p] | ((unsigned)px[3 * p + 1] << 8) | ((unsigned)px[3 * p + 2] << 16);
}
// the pixel of the head / tail that thread `tid` of a frame's first workgroup takes, -1 for none
__device__ __forceinline__ long long lbl_edge_pixel(const LblSpan& s, int tid) {
  if (tid < s.head) return tid;
  if (tid >= 4 && tid - 4 < s.tail) return s.head + 4 * s.groups + (tid - 4);
  return -1;
}
struct LblKeys {
  unsigned k[4];
};
__device__ __forceinline__ LblKeys lbl_group_keys(const LblSpan& s, long long g) {
  struct __attribute__((aligned(4))) U3 {
    unsigned a, b, c;
  };
  const U3 d = *reinterpret_cast<const U3*>(s.px + 3 * (long long)s.head + 12 * g);
  LblKeys r;
  r.k[0] = d.a & 0xffffffu;
  r.k[1] = (d.a >> 24) | ((d.b & 0xffffu) << 8);
  r.k[2] = (d.b >> 16) | ((d.c & 0xffu) << 16);
  r.k[3] = d.c >> 8;
  return r;
}

// key into an open-addressing set of LBL_SLOTS words (0 = empty; a key is never 0).  0: was there, 1: inserted, -1: the set
// is full.  At most LBL_SLOTS probes.
__device__ __forceinline__ int lbl_set_insert(unsigned* set, unsigned key) {
  unsigned s = lbl_hash(key);
  for (int i = 0; i < LBL_SLOTS; ++i, s = (s + 1) & (LBL_SLOTS - 1)) {
    unsigned old = __hip_atomic_load(&set[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == key) return 0;
    if (old != 0u) continue;
    old = atomicCAS(&set[s], 0u, key);
    if (old == 0u) return 1;
    if (old == key) return 0;
  }
  return -1;
}

__global__ void __launch_bounds__(256) labels_collect_kernel(const uint8_t* frames, long long hw, int bpf, unsigned* ws) {
  __shared__ unsigned set[LBL_SLOTS];
  __shared__ unsigned count, over;
  const int tid = threadIdx.x;
  const long long f = blockIdx.x / bpf;
  const int b = blockIdx.x % bpf;
  unsigned* table = ws + f * (LBL_SLOTS + LBL_HDR);
  for (int i = tid; i < LBL_SLOTS; i += 256) set[i] = 0u;
  if (tid == 0) {
    count = 0u;
    over = 0u;
  }
  __syncthreads();
  volatile unsigned* vover = &over;
  auto add = [&](unsigned key) {  // more than 255 keys in one workgroup's pixels: the frame overflows whatever the others hold
    const int r = lbl_set_insert(set, key);
    if (r < 0 || (r > 0 && atomicAdd(&count, 1u) >= LBL_MAX)) *vover = 1u;
  };
  const LblSpan s = lbl_span(frames, f, hw);
  if (b == 0) {
    const long long p = lbl_edge_pixel(s, tid);
    if (p >= 0) {
      const unsigned k = lbl_key_at(s.px, p);
      if (k) add(k);
    }
  }
  unsigned last = 0u;
  for (long long g = b * 256LL + tid; g < s.groups; g += bpf * 256LL) {
    if (*vover) break;
    const LblKeys q = lbl_group_keys(s, g);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (q.k[j] != last) {
        last = q.k[j];
        if (last) add(last);
      }
    }
  }
  __syncthreads();
  if (*vover) {
    if (tid == 0) atomicOr(&table[LBL_SLOTS], 1u);
    return;
  }
  for (int i = tid; i < LBL_SLOTS; i += 256) {
    const unsigned k = set[i];
    if (k && lbl_set_insert(table, k) < 0) atomicOr(&table[LBL_SLOTS], 1u);
  }
}

__global__ void __launch_bounds__(256) labels_rank_kernel(const unsigned* ws, unsigned* colors, int* num_colors) {
  __shared__ unsigned keys[256], out[256];
  __shared__ unsigned n_found;
  const int tid = threadIdx.x;
  const long long f = blockIdx.x;
  const unsigned* table = ws + f * (LBL_SLOTS + LBL_HDR);
  if (tid == 0) n_found = 0u;
  out[tid] = 0u;
  __syncthreads();
  for (int i = tid; i < LBL_SLOTS; i += 256) {
    const unsigned k = table[i];
    if (k) {
      const unsigned at = atomicAdd(&n_found, 1u);
      if (at < 256u) keys[at] = k;
    }
  }
  __syncthreads();
  const unsigned n = n_found;
  const bool over = table[LBL_SLOTS] != 0u || n > LBL_MAX;
  if (!over && (unsigned)tid < n) {  // the slot order above is arbitrary; the rank of a key's VALUE is not
    const unsigned k = keys[tid];
    unsigned rank = 0u;
    for (unsigned j = 0; j < n; ++j) rank += keys[j] < k ? 1u : 0u;
    out[rank + 1u] = k;
  }
  __syncthreads();
  colors[f * 256 + tid] = out[tid];
  if (tid == 0) num_colors[f] = over ? 256 : (int)n;
}

__global__ void __launch_bounds__(256) labels_apply_kernel(const uint8_t* frames, long long hw, int bpf, const unsigned* colors,
                                                          const int* num_colors, uint8_t* labels) {
  __shared__ unsigned map[LBL_SLOTS];  // label << 24 | key, 0 = empty
  const int tid = threadIdx.x;
  const long long f = blockIdx.x / bpf;
  const int b = blockIdx.x % bpf;
  const int n = num_colors[f];
  if (n < 0 || n > (int)LBL_MAX) return;  // an overflowed frame keeps whatever its label bytes held
  for (int i = tid; i < LBL_SLOTS; i += 256) map[i] = 0u;
  __syncthreads();
  if (tid < n) {
    const unsigned key = colors[f * 256 + tid + 1] & 0xffffffu;
    const unsigned entry = ((unsigned)(tid + 1) << 24) | key;
    unsigned s = lbl_hash(key);
    for (int i = 0; i < LBL_SLOTS; ++i, s = (s + 1) & (LBL_SLOTS - 1))
      if (atomicCAS(&map[s], 0u, entry) == 0u) break;
  }
  __syncthreads();
  auto find = [&](unsigned key) -> unsigned {
    unsigned s = lbl_hash(key);
    for (int i = 0; i < LBL_SLOTS; ++i, s = (s + 1) & (LBL_SLOTS - 1)) {
      const unsigned e = map[s];
      if (e == 0u) return 0u;
      if ((e & 0xffffffu) == key) return e >> 24;
    }
    return 0u;
  };
  const LblSpan s = lbl_span(frames, f, hw);
  uint8_t* dst = labels + f * hw;
  if (b == 0) {
    const long long p = lbl_edge_pixel(s, tid);
    if (p >= 0) {
      const unsigned k = lbl_key_at(s.px, p);
      dst[p] = (uint8_t)(k ? find(k) : 0u);
    }
  }
  uint8_t* body = dst + s.head;
  const bool aligned = (reinterpret_cast<uintptr_t>(body) & 3) == 0;  // uniform over the frame
  unsigned last = 0u, last_label = 0u;
  for (long long g = b * 256LL + tid; g < s.groups; g += bpf * 256LL) {
    const LblKeys q = lbl_group_keys(s, g);
    unsigned packed = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (q.k[j] != last) {
        last = q.k[j];
        last_label = last ? find(last) : 0u;
      }
      packed |= last_label << (8 * j);
    }
    if (aligned) {
      *reinterpret_cast<unsigned*>(body + 4 * g) = packed;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) body[4 * g + j] = (uint8_t)(packed >> (8 * j));
    }
  }
}

}  // namespace cn

extern "C" size_t cn_instance_labels_workspace_bytes(int32_t num_frames) {
  return num_frames <= 0 ? 0 : (size_t)num_frames * (cn::LBL_SLOTS + cn::LBL_HDR) * sizeof(uint32_t);
}

extern "C" int cn_instance_labels(const uint8_t* frames, int32_t num_frames, int32_t height, int32_t width, uint8_t* labels,
                                  uint32_t* colors, int32_t* num_colors, void* workspace, size_t workspace_bytes,
                                  cn_stream_t stream) {
  CN_REQUIRE(num_frames >= 0 && height >= 0 && width >= 0, CN_ERR_INVALID, "cn_instance_labels: %d frames of %d x %d",
             num_frames, height, width);
  const long long hw = (long long)height * width;
  if (num_frames == 0 || hw == 0) return CN_OK;
  CN_REQUIRE(frames && labels && colors && num_colors && workspace, CN_ERR_INVALID, "cn_instance_labels: null argument");
  CN_REQUIRE(workspace_bytes >= cn_instance_labels_workspace_bytes(num_frames), CN_ERR_INVALID,
             "cn_instance_labels: workspace %zu B < %zu B", workspace_bytes, cn_instance_labels_workspace_bytes(num_frames));
  CN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0 && (reinterpret_cast<uintptr_t>(colors) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(num_colors) & 3) == 0,
             CN_ERR_INVALID, "cn_instance_labels: workspace, colors and num_colors must be 4-B aligned");
  // 8 groups of four pixels per thread amortise a workgroup's set; at most 512 workgroups feed one frame's table
  long long bpf = (hw / 4 + 256 * 8 - 1) / (256 * 8);
  bpf = bpf < 1 ? 1 : (bpf > 512 ? 512 : bpf);
  CN_REQUIRE(bpf * num_frames < (1LL << 31), CN_ERR_UNSUPPORTED, "cn_instance_labels: %d frames of %d x %d in one call",
             num_frames, height, width);
  hipStream_t s = cn::as_stream(stream);
  unsigned* ws = static_cast<unsigned*>(workspace);
  const hipError_t e = hipMemsetAsync(ws, 0, cn_instance_labels_workspace_bytes(num_frames), s);  // the tables, at every call
  CN_REQUIRE(e == hipSuccess, CN_ERR_LAUNCH, "cn_instance_labels: clearing the tables: %s", hipGetErrorString(e));
  const dim3 grid((unsigned)(bpf * num_frames));
  hipLaunchKernelGGL(cn::labels_collect_kernel, grid, dim3(256), 0, s, frames, hw, (int)bpf, ws);
  hipLaunchKernelGGL(cn::labels_rank_kernel, dim3(num_frames), dim3(256), 0, s, ws, colors, num_colors);
  hipLaunchKernelGGL(cn::labels_apply_kernel, grid, dim3(256), 0, s, frames, hw, (int)bpf, colors, num_colors, labels);
  return cn::check_launch("cn_instance_labels");
}
