// Connected components of a label volume slab by slab: what joins the per-slab results of emp_ccl_range (sparse.hip) into the
// components of the whole array.
//
// A slab's CCL numbers its components 1..K in raster order of their first voxels.  Offset by the number of components of the slabs
// before it (the slab's base), these are provisional ids 1..G in which a smaller id always starts earlier in raster order.  The
// three entries work on that id space with the invariant of the voxel kernels (union_find.h): a root is the smallest id of its
// set, so ranking the roots in id order IS raster order of the first voxels of the whole array's components.
//   emp_ccl_seam        unions across the seam between two slabs: a voxel of the current slab's first slice with its up to 9
//                       neighbours of equal value in the previous slab's last slice
//   emp_ccl_rank_roots  flatten / count / scan / rank over the ids, as ccl_run does over voxels -> lut[provisional id] = final number
//   emp_ccl_lut         out = lut[base + local id] per voxel of a slab
#include "common.h"
#include "union_find.h"

namespace emp {
namespace {

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    uint32_t t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}
// exclusive scan over the 256 threads of a block; *total: the block's sum.  sh: 4 words of LDS
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* sh, uint32_t* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t inc = wave_incl_scan(v, lane);
  __syncthreads();
  if (lane == 63) sh[w] = inc;
  __syncthreads();
  uint32_t base = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < w) base += sh[i];
  *total = sh[0] + sh[1] + sh[2] + sh[3];
  return base + inc - v;
}

// One thread per voxel of the current slab's first slice, consecutive x per lane.  A voxel with a local id (non-zero: its value
// lies in the range the slab's CCL kept) is united with the voxels of the previous slab's last slice that hold the same value and
// an id.  The previous slice's own CCL has joined its in-plane neighbours already, and all nine candidates are in-plane
// neighbours of the one straight below: where that one matches, its union is all nine.
template <typename T>
__global__ void __launch_bounds__(256) ccl_seam_kernel(const T* __restrict__ pv, const int32_t* __restrict__ pid,
                                                       const T* __restrict__ cv, const int32_t* __restrict__ cid, int h, int w,
                                                       int base_prev, int base_cur, int* __restrict__ parent, int64_t n_parent) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= h * w) return;
  const int32_t id = cid[p];
  if (id == 0) return;
  const int64_t a = (int64_t)base_cur + id;
  if (a <= 0 || a >= n_parent) return;      // not an id of `parent`: the caller's bases are wrong; never index past the array
  const T v = cv[p];
  const int y = p / w, x = p - y * w;
  auto join = [&](int q) {
    const int32_t jd = pid[q];
    if (jd == 0 || pv[q] != v) return false;
    const int64_t b = (int64_t)base_prev + jd;
    if (b > 0 && b < n_parent) uf_union(parent, (int)a, (int)b);
    return true;
  };
  if (join(p)) return;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
    if ((unsigned)(y + dy) >= (unsigned)h) continue;
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      if ((dy == 0 && dx == 0) || (unsigned)(x + dx) >= (unsigned)w) continue;
      join(p + dy * w + dx);
    }
  }
}

// ids 1..g; entry 0 is the background's and stays out of everything
__global__ void __launch_bounds__(256) cc_flatten_kernel(int* __restrict__ parent, int64_t g) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
  if (i <= g) parent[i] = uf_find(parent, (int)i);
}

constexpr int CHUNK = 2048;      // ids per block of the count and rank kernels: 8 per thread
__global__ void __launch_bounds__(256) cc_count_kernel(const int* __restrict__ parent, int64_t g, uint32_t* __restrict__ blockcnt) {
  __shared__ uint32_t sh[4];
  const int64_t e0 = (int64_t)blockIdx.x * CHUNK + threadIdx.x * 8;
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int64_t i = e0 + j;
    if (i >= 1 && i <= g && parent[i] == (int)i) ++c;
  }
  uint32_t total;
  block_excl_scan(c, sh, &total);
  if (threadIdx.x == 0) blockcnt[blockIdx.x] = total;
}
__global__ void __launch_bounds__(256) cc_scan_blocks_kernel(const uint32_t* __restrict__ blockcnt, uint32_t* __restrict__ blockoff,
                                                             int nb, int32_t* __restrict__ total_out) {
  __shared__ uint32_t sh[4];
  uint32_t carry = 0;
  for (int b0 = 0; b0 < nb; b0 += 256) {
    const int b = b0 + threadIdx.x;
    const uint32_t c = b < nb ? blockcnt[b] : 0;
    uint32_t t;
    const uint32_t e = block_excl_scan(c, sh, &t);
    if (b < nb) blockoff[b] = carry + e;
    carry += t;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total_out = (int32_t)carry;
}
// lut[root] = its 1-based rank among the roots, in id order
__global__ void __launch_bounds__(256) cc_rank_kernel(const int* __restrict__ parent, int64_t g, const uint32_t* __restrict__ blockoff,
                                                      int32_t* __restrict__ lut) {
  __shared__ uint32_t sh[4];
  const int64_t e0 = (int64_t)blockIdx.x * CHUNK + threadIdx.x * 8;
  uint32_t c = 0, flags = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int64_t i = e0 + j;
    if (i >= 1 && i <= g && parent[i] == (int)i) { ++c; flags |= 1u << j; }
  }
  uint32_t total;
  uint32_t pos = block_excl_scan(c, sh, &total) + blockoff[blockIdx.x];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (flags & (1u << j)) lut[e0 + j] = (int32_t)(++pos);
}
// every other id takes its root's number: the roots' entries are only read here, the others only written
__global__ void __launch_bounds__(256) cc_spread_kernel(const int* __restrict__ parent, int64_t g, int32_t* __restrict__ lut) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > g) return;
  if (i == 0) { lut[0] = 0; return; }
  const int r = parent[i];
  if (r != (int)i) lut[i] = (r >= 1 && r < i) ? lut[r] : 0;      // a root is the smallest id of its set; anything else is no forest
}

__global__ void __launch_bounds__(256) cc_lut_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ lut, int64_t base,
                                                     int64_t n_lut, int32_t* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int32_t id = ids[i];
    const int64_t g = base + id;
    out[i] = (id > 0 && g < n_lut) ? lut[g] : 0;
  }
}

}  // namespace
}  // namespace emp

using namespace emp;

extern "C" {

int emp_ccl_seam(const void* d_prev_vals, const int32_t* d_prev_ids, const void* d_cur_vals, const int32_t* d_cur_ids, int in_bytes,
                 int H, int W, int64_t base_prev, int64_t base_cur, int32_t* d_parent, int64_t n_parent, void* stream) {
  EMP_REQUIRE(d_prev_vals && d_prev_ids && d_cur_vals && d_cur_ids && d_parent && H > 0 && W > 0, "ccl_seam: bad arguments");
  EMP_REQUIRE(in_bytes == 4 || in_bytes == 8, "ccl_seam: 4- or 8-byte labels, as emp_ccl_range reads them");
  EMP_REQUIRE((int64_t)H * W < (1ll << 30), "ccl_seam: slice too large (< 2^30 elements)");
  EMP_REQUIRE(base_prev >= 0 && base_cur >= base_prev && n_parent > base_cur && n_parent <= (1ll << 31) - 1,
              "ccl_seam: 0 <= base_prev <= base_cur < n_parent < 2^31");
  const int hw = H * W;
  hipStream_t s = (hipStream_t)stream;
  if (in_bytes == 8)
    hipLaunchKernelGGL(ccl_seam_kernel<int64_t>, dim3(cdiv(hw, 256)), dim3(256), 0, s, (const int64_t*)d_prev_vals, d_prev_ids,
                       (const int64_t*)d_cur_vals, d_cur_ids, H, W, (int)base_prev, (int)base_cur, d_parent, n_parent);
  else
    hipLaunchKernelGGL(ccl_seam_kernel<int32_t>, dim3(cdiv(hw, 256)), dim3(256), 0, s, (const int32_t*)d_prev_vals, d_prev_ids,
                       (const int32_t*)d_cur_vals, d_cur_ids, H, W, (int)base_prev, (int)base_cur, d_parent, n_parent);
  EMP_LAUNCH_CHECK();
  return EMP_OK;
}

size_t emp_ccl_rank_roots_work_bytes(int64_t G) {
  if (G < 0 || G > (1ll << 31) - 2) return 0;
  const size_t nb = (size_t)((G + 1 + CHUNK - 1) / CHUNK);
  return nb * 8 + 256;
}

int emp_ccl_rank_roots(int32_t* d_parent, int64_t G, int32_t* d_lut, int32_t* d_count, void* d_work, void* stream) {
  EMP_REQUIRE(d_parent && d_lut && d_count && d_work, "ccl_rank_roots: bad arguments");
  EMP_REQUIRE(G >= 0 && G <= (1ll << 31) - 2, "ccl_rank_roots: 0 <= G <= 2^31 - 2");
  hipStream_t s = (hipStream_t)stream;
  const int nb = (int)((G + 1 + CHUNK - 1) / CHUNK);
  const int nt = (int)((G + 1 + 255) / 256);
  uint32_t* blockcnt = (uint32_t*)d_work;
  uint32_t* blockoff = blockcnt + nb;
  if (G > 0) {
    hipLaunchKernelGGL(cc_flatten_kernel, dim3((int)((G + 255) / 256)), dim3(256), 0, s, d_parent, G);
    EMP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(cc_count_kernel, dim3(nb), dim3(256), 0, s, d_parent, G, blockcnt);
  EMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_scan_blocks_kernel, dim3(1), dim3(256), 0, s, blockcnt, blockoff, nb, d_count);
  EMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_rank_kernel, dim3(nb), dim3(256), 0, s, d_parent, G, blockoff, d_lut);
  EMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_spread_kernel, dim3(nt), dim3(256), 0, s, d_parent, G, d_lut);
  EMP_LAUNCH_CHECK();
  return EMP_OK;
}

int emp_ccl_lut(const int32_t* d_ids, const int32_t* d_lut, int64_t base, int64_t n_lut, int32_t* d_out, int64_t n, void* stream) {
  EMP_REQUIRE(d_ids && d_lut && d_out && n >= 0 && base >= 0 && n_lut > base && n_lut <= (1ll << 31) - 1, "ccl_lut: bad arguments");
  if (n == 0) return EMP_OK;
  int64_t grid = (n + 255) / 256;
  if (grid > 256 * 64) grid = 256 * 64;
  hipLaunchKernelGGL(cc_lut_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, d_ids, d_lut, base, n_lut, d_out, n);
  EMP_LAUNCH_CHECK();
  return EMP_OK;
}

}  // extern "C"
