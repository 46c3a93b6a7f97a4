// PointRend subdivision inference for gfx950 (reference:
// empanada/models/point_rend.py:241-269, eval branch):
//   per step: x2 bilinear upsample (align_corners=False) of the logits,
//   uncertainty (-|logit| or top2 difference, :11-31), the num_points most
//   uncertain grid cells (torch.topk, :123-137), bilinear point sampling of the
//   coarse logits and of the decoder features (grid_sample, :33-60), a 3-layer
//   point MLP (runs on the implicit-GEMM kernel as a 1x1 conv over the point
//   list) and a scatter of the refined logits back into the grid.
// Top-k is an exact radix select on the fp32 bit pattern of a non-negative key
// (smaller key = more uncertain) followed by an ORDERED compaction, so the
// selected set is deterministic: all keys below the k-th value, plus the
// lowest-index cells among those equal to it.  Two forms with the same output:
// the two-read select (default, "Two-read select" below) and the four-pass
// select that reads the keys six times (EMP_TOPK_LEGACY=1).
#include "common.h"

namespace emp {
namespace {

constexpr int CHUNK = 2048;  // elements per block in the select / compact passes

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    uint32_t t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}
// exclusive scan over the 256 threads of a block; *total gets the block sum
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* sh /*[5]*/, uint32_t* total) {
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

// One x2 sample (align_corners=False) in the operation order the compiler's contraction gave the first form of this kernel
// (read from its gfx950 code): t0 = fma(lx, v01, hx * v00), t1 = fma(hx, v10, lx * v11), v = hy * t0 + ly * t1 with a plain
// add.  Written out under fp contract(off) so that the one-output and the four-output kernel agree by construction.
__device__ __forceinline__ float up2x_sample(float v00, float v01, float v10, float v11, float hx, float lx, float hy, float ly) {
#pragma clang fp contract(off)
  const float t0 = __builtin_fmaf(lx, v01, hx * v00);
  const float t1 = __builtin_fmaf(hx, v10, lx * v11);
  const float a = hy * t0, b = ly * t1;
  return a + b;
}
// source coordinate of output o: 0.5 * (o + 0.5) - 0.5 clamped at 0 (the product by 0.5 is exact: fused or not, the same bits)
__device__ __forceinline__ float up2x_coord(int o) {
#pragma clang fp contract(off)
  const float f = 0.5f * ((float)o + 0.5f) - 0.5f;
  return f < 0.f ? 0.f : f;
}

// EMP_PR_UP2X_LEGACY=1: one output per thread, grid-stride
__global__ void __launch_bounds__(256) upsample2x_keys_kernel(const float* __restrict__ in, int N, int C, int h, int w,
                                                              float* __restrict__ out, uint32_t* __restrict__ keys,
                                                              int64_t total) {
#pragma clang fp contract(off)
  const int H = 2 * h, W = 2 * w;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int ox = (int)(i % W);
    int64_t p = i / W;
    int oy = (int)(p % H);
    int n = (int)(p / H);
    const float fy = up2x_coord(oy), fx = up2x_coord(ox);
    int y0 = (int)fy, x0 = (int)fx;
    int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    float ly = fy - (float)y0, lx = fx - (float)x0;
    float hy = 1.f - ly, hx = 1.f - lx;
    float top1 = -INFINITY, top2 = -INFINITY, v0 = 0.f;
    for (int c = 0; c < C; ++c) {
      const float* b = in + ((size_t)n * C + c) * h * w;
      float v = up2x_sample(b[y0 * w + x0], b[y0 * w + x1], b[y1 * w + x0], b[y1 * w + x1], hx, lx, hy, ly);
      out[(((size_t)n * C + c) * H + oy) * W + ox] = v;
      if (c == 0) v0 = v;
      if (v > top1) { top2 = top1; top1 = v; } else if (v > top2) { top2 = v; }
    }
    float key = (C == 1) ? fabsf(v0) : (top1 - top2);
    keys[i] = __float_as_uint(key);
  }
}

// A thread produces outputs 4q .. 4q + 3 of one row: their source columns are 2q - 1 .. 2q + 2 (clamped into the row), so eight
// loads per class feed one 16-byte store of logits and, after the last class, one of keys; 32-bit indices (the entry bounds
// N * 4hw below 2^31), one row group per thread, no loop over the grid.  VEC 4: 16-byte stores (W % 4 == 0, both bases on a
// 16-byte boundary); VEC 2: 8-byte stores (W is even; odd w ends each row in a pair); VEC 1: guarded 4-byte stores.
template <int VEC>
__global__ void __launch_bounds__(256) upsample2x_keys4_kernel(const float* __restrict__ in, int C, int h, int w,
                                                               float* __restrict__ out, uint32_t* __restrict__ keys,
                                                               int Wq, int total) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int H = 2 * h, W = 2 * w;
  const int q = i % Wq, row = i / Wq;
  const int oy = row % H, n = row / H;
  const float fy = up2x_coord(oy);
  const int y0 = (int)fy, y1 = y0 + (y0 < h - 1 ? 1 : 0);
  const float ly = fy - (float)y0, hy = 1.f - ly;
  int xc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = 2 * q - 1 + k;
    xc[k] = x < 0 ? 0 : (x < w - 1 ? x : w - 1);
  }
  float lx[4], hx[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float fx = up2x_coord(4 * q + j);
    lx[j] = fx - (float)(int)fx;
    hx[j] = 1.f - lx[j];
  }
  const bool first = q == 0;                       // output 0: x0 = 0, x1 = min(1, w - 1) are columns 1 and 2 of the four
  const int valid = W - 4 * q < 4 ? W - 4 * q : 4; // 2 in the last group of a row with odd w
  float top1[4], top2[4], v0[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { top1[j] = -INFINITY; top2[j] = -INFINITY; v0[j] = 0.f; }
  const int plane = h * w, oplane = H * W;
  const float* b = in + (size_t)n * C * plane;
  float* o = out + (size_t)n * C * oplane + oy * W + 4 * q;
  for (int c = 0; c < C; ++c, b += plane, o += oplane) {
    float r0[4], r1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { r0[k] = b[y0 * w + xc[k]]; r1[k] = b[y1 * w + xc[k]]; }
    float v[4];
    v[0] = up2x_sample(first ? r0[1] : r0[0], first ? r0[2] : r0[1], first ? r1[1] : r1[0], first ? r1[2] : r1[1], hx[0], lx[0], hy, ly);
    v[1] = up2x_sample(r0[1], r0[2], r1[1], r1[2], hx[1], lx[1], hy, ly);
    v[2] = up2x_sample(r0[1], r0[2], r1[1], r1[2], hx[2], lx[2], hy, ly);
    v[3] = up2x_sample(r0[2], r0[3], r1[2], r1[3], hx[3], lx[3], hy, ly);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (c == 0) v0[j] = v[j];
      if (v[j] > top1[j]) { top2[j] = top1[j]; top1[j] = v[j]; } else if (v[j] > top2[j]) { top2[j] = v[j]; }
    }
    if (VEC == 4) {
      *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else if (VEC == 2) {
      *reinterpret_cast<float2*>(o) = make_float2(v[0], v[1]);
      if (valid == 4) *reinterpret_cast<float2*>(o + 2) = make_float2(v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < valid) o[j] = v[j];
    }
  }
  uint32_t key[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) key[j] = __float_as_uint((C == 1) ? fabsf(v0[j]) : (top1[j] - top2[j]));
  uint32_t* kp = keys + (size_t)row * W + 4 * q;
  if (VEC == 4) {
    *reinterpret_cast<uint4*>(kp) = make_uint4(key[0], key[1], key[2], key[3]);
  } else if (VEC == 2) {
    *reinterpret_cast<uint2*>(kp) = make_uint2(key[0], key[1]);
    if (valid == 4) *reinterpret_cast<uint2*>(kp + 2) = make_uint2(key[2], key[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < valid) kp[j] = key[j];
  }
}

// state[n] = {prefix, k_remaining, unused, unused}
__global__ void init_state_kernel(uint32_t* state, uint32_t* hist, int N, uint32_t k) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i < N) { state[4 * i] = 0; state[4 * i + 1] = k; state[4 * i + 2] = 0; state[4 * i + 3] = 0; }
  if (i < N * 256) hist[i] = 0;
}

__global__ void __launch_bounds__(256) radix_hist_kernel(const uint32_t* __restrict__ keys, int64_t plane,
                                                         const uint32_t* __restrict__ state,
                                                         uint32_t* __restrict__ hist, int shift, uint32_t himask) {
  __shared__ uint32_t lh[256];
  const int n = blockIdx.y;
  lh[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t prefix = state[4 * n];
  const uint32_t* kp = keys + (size_t)n * plane;
  const int64_t base = (int64_t)blockIdx.x * CHUNK;
#pragma unroll
  for (int j = 0; j < CHUNK / 256; ++j) {
    int64_t i = base + j * 256 + threadIdx.x;
    if (i < plane) {
      uint32_t k = kp[i];
      if ((k & himask) == prefix) atomicAdd(&lh[(k >> shift) & 255u], 1u);
    }
  }
  __syncthreads();
  uint32_t c = lh[threadIdx.x];
  if (c) atomicAdd(&hist[n * 256 + threadIdx.x], c);
}

__global__ void __launch_bounds__(256) radix_select_kernel(uint32_t* __restrict__ hist, uint32_t* __restrict__ state,
                                                           int shift) {
  __shared__ uint32_t sh[8];
  const int n = blockIdx.x;
  uint32_t c = hist[n * 256 + threadIdx.x];
  hist[n * 256 + threadIdx.x] = 0;
  uint32_t total;
  uint32_t ex = block_excl_scan(c, sh, &total);
  const uint32_t krem = state[4 * n + 1];
  const uint32_t prefix = state[4 * n];
  __syncthreads();
  if (c > 0 && ex < krem && krem <= ex + c) {
    state[4 * n] = prefix | ((uint32_t)threadIdx.x << shift);
    state[4 * n + 1] = krem - ex;
  }
}

__device__ __forceinline__ uint32_t count_flags(const uint32_t* kp, int64_t plane, int64_t e0, uint32_t T,
                                                uint32_t* flags_less, uint32_t* flags_eq) {
  // thread handles 8 consecutive elements starting at e0; returns less | eq<<16
  uint32_t fl = 0, fe = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int64_t i = e0 + j;
    if (i < plane) {
      uint32_t k = kp[i];
      fl |= (uint32_t)(k < T) << j;
      fe |= (uint32_t)(k == T) << j;
    }
  }
  *flags_less = fl;
  *flags_eq = fe;
  return (uint32_t)__popc(fl) | ((uint32_t)__popc(fe) << 16);
}

__global__ void __launch_bounds__(256) compact_count_kernel(const uint32_t* __restrict__ keys, int64_t plane,
                                                            const uint32_t* __restrict__ state,
                                                            uint32_t* __restrict__ blockcnt, int nb) {
  __shared__ uint32_t sh[8];
  const int n = blockIdx.y;
  const uint32_t T = state[4 * n];
  uint32_t fl, fe;
  uint32_t c = count_flags(keys + (size_t)n * plane, plane, (int64_t)blockIdx.x * CHUNK + threadIdx.x * 8, T, &fl, &fe);
  uint32_t total;
  block_excl_scan(c, sh, &total);
  if (threadIdx.x == 0) blockcnt[(size_t)n * nb + blockIdx.x] = total;
}

// exclusive scan of the per-block (less | eq<<16) counts -> 2 x uint32 offsets
__global__ void __launch_bounds__(256) compact_scan_kernel(const uint32_t* __restrict__ blockcnt,
                                                           uint32_t* __restrict__ blockoff, int nb) {
  __shared__ uint32_t sh[8];
  const int n = blockIdx.x;
  uint32_t carry_l = 0, carry_e = 0;
  for (int b0 = 0; b0 < nb; b0 += 256) {
    int b = b0 + threadIdx.x;
    uint32_t c = b < nb ? blockcnt[(size_t)n * nb + b] : 0;
    uint32_t tl, te;
    uint32_t el = block_excl_scan(c & 0xffffu, sh, &tl);
    uint32_t ee = block_excl_scan(c >> 16, sh, &te);
    if (b < nb) {
      blockoff[((size_t)n * nb + b) * 2] = carry_l + el;
      blockoff[((size_t)n * nb + b) * 2 + 1] = carry_e + ee;
    }
    carry_l += tl;
    carry_e += te;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) compact_write_kernel(const uint32_t* __restrict__ keys, int64_t plane,
                                                            const uint32_t* __restrict__ state,
                                                            const uint32_t* __restrict__ blockoff, int nb, int k,
                                                            int32_t* __restrict__ idx_out) {
  __shared__ uint32_t sh[8];
  const int n = blockIdx.y;
  const uint32_t T = state[4 * n];
  const uint32_t krem = state[4 * n + 1];
  const uint32_t nless = (uint32_t)k - krem;
  const int64_t e0 = (int64_t)blockIdx.x * CHUNK + threadIdx.x * 8;
  uint32_t fl, fe;
  uint32_t c = count_flags(keys + (size_t)n * plane, plane, e0, T, &fl, &fe);
  uint32_t tl, te;
  uint32_t pl = block_excl_scan(c & 0xffffu, sh, &tl) + blockoff[((size_t)n * nb + blockIdx.x) * 2];
  uint32_t pe = block_excl_scan(c >> 16, sh, &te) + blockoff[((size_t)n * nb + blockIdx.x) * 2 + 1];
  int32_t* o = idx_out + (size_t)n * k;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (fl & (1u << j)) { o[pl++] = (int32_t)(e0 + j); }
    if (fe & (1u << j)) {
      if (pe < krem) o[nless + pe] = (int32_t)(e0 + j);
      ++pe;
    }
  }
}

// ---------------------------------------------------------------------------
// Two-read select (default; EMP_TOPK_LEGACY=1 takes the four-pass kernels above).  The keys are read twice, 16 bytes per lane:
//   digit pass     per-image histogram of the SEL_BITS bits below the sign bit (bit 31 of a non-negative float is 0);
//                  sel_find_kernel finds the threshold bin B, the count still to take from it and whether the bin fits the
//                  candidate buffer (SEL_CAP keys);
//   candidate pass keys whose digit is below B are selected outright: one bit per key in the `less` mask; keys in bin B set
//                  their bit in the `eq` mask and go, with their index, to the image's candidate buffer; per-chunk counts of
//                  both masks as in the legacy compaction;
//   resolve        one workgroup per image: the exact 32-bit threshold T by bisection over the candidates in registers; the
//                  candidates below T move to the `less` mask, those above T leave the `eq` mask (atomics on the few words and
//                  chunk counts concerned), then the exclusive scan of the chunk counts;
//   ordered write  compact_write_kernel's arithmetic on the two masks: the keys are not read again.
// An image whose threshold bin holds more than SEL_CAP keys (a constant image: padding, a blank slice) sets its overflow
// flag on the device and refines the threshold with two more histogram levels (bits 18..7, bits 6..0: launches whose
// workgroups return at once for every other image); the candidate pass then compares such an image's keys with the exact
// T and appends nothing: five reads, against the six of the legacy select.  No host synchronisation; a batch may mix both.
// Alignment: an image's keys start s = (address / 4) & 3 elements past a 16-byte boundary.  Every pass indexes the image by
// v = i + s, so that the group v / 4 is one aligned uint4; the groups that hold v < s or v >= plane + s are read by guarded
// scalar loads.  Masks, chunk counts and candidate indices are in v; the ordered write subtracts s.
// state[n] = {prefix / T, k remaining, overflow, candidates, unused x 4}
// ---------------------------------------------------------------------------
constexpr int SEL_BITS = 12;                       // width of the leading digit (bits 30..19)
constexpr int SEL_CAP = 8192;                      // candidate keys per image
constexpr int SEL_BINS = 1 << SEL_BITS;
constexpr int SEL_SHIFT = 31 - SEL_BITS;           // 19
constexpr int SEL_L2_BITS = 12, SEL_L2_SHIFT = SEL_SHIFT - SEL_L2_BITS;      // overflow level 2: bits 18..7
constexpr int SEL_HIST_CHUNKS = 4;                 // chunks of CHUNK keys per workgroup of the histogram pass
constexpr int SEL_STATE = 8;
constexpr int SEL_WORDS = CHUNK / 32;              // mask words per chunk

__device__ __forceinline__ uint32_t sel_shift_of(const uint32_t* kp) { return (uint32_t)(((uintptr_t)kp >> 2) & 3u); }

// the four keys of group g (v = 4g .. 4g + 3) of an image; ok = bit j set where v is a key of the image
__device__ __forceinline__ uint4 sel_load4(const uint32_t* __restrict__ kp, int64_t plane, uint32_t sh, int64_t g,
                                           uint32_t* ok) {
  const int64_t i0 = 4 * g - (int64_t)sh;
  if (i0 >= 0 && i0 + 3 < plane) {
    *ok = 15u;
    return *reinterpret_cast<const uint4*>(kp + i0);
  }
  uint32_t k[4], m = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t i = i0 + j;
    const bool in = i >= 0 && i < plane;
    k[j] = in ? kp[in ? i : 0] : 0u;
    m |= (uint32_t)in << j;
  }
  *ok = m;
  return make_uint4(k[0], k[1], k[2], k[3]);
}

__global__ void sel_init_kernel(uint32_t* __restrict__ state, uint32_t* __restrict__ hist, int N, uint32_t k) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < N * SEL_STATE) state[i] = (i % SEL_STATE) == 1 ? k : 0u;
  if (i < N * SEL_BINS) hist[i] = 0;
}

// one workgroup per image: the bin that holds the k-th key; the histogram is left zeroed for the next level
__global__ void __launch_bounds__(256) sel_find_kernel(uint32_t* __restrict__ hist, uint32_t* __restrict__ state, int level,
                                                       int shift) {
  __shared__ uint32_t sh[8];
  const int n = blockIdx.x;
  if (level > 0 && state[SEL_STATE * n + 2] == 0) return;
  constexpr int PER = SEL_BINS / 256;
  uint32_t c[PER], sum = 0;
  uint32_t* h = hist + (size_t)n * SEL_BINS + threadIdx.x * PER;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    c[j] = h[j];
    h[j] = 0;
    sum += c[j];
  }
  uint32_t total;
  uint32_t ex = block_excl_scan(sum, sh, &total);
  const uint32_t krem = state[SEL_STATE * n + 1];
  const uint32_t prefix = state[SEL_STATE * n];
  __syncthreads();
  if (sum > 0 && ex < krem && krem <= ex + sum) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (c[j] > 0 && ex < krem && krem <= ex + c[j]) {
        state[SEL_STATE * n] = prefix | ((uint32_t)(threadIdx.x * PER + j) << shift);
        state[SEL_STATE * n + 1] = krem - ex;
        if (level == 0) state[SEL_STATE * n + 2] = c[j] > (uint32_t)SEL_CAP ? 1u : 0u;
      }
      ex += c[j];
    }
  }
}

// level 0: every image, digit = bits 30..19.  levels 1, 2: overflow images only, keys that match the prefix found so far.
// [measured on the bench's keys, both stages of a step: plain LDS atomics, one per key, 45 us; electing one lane per
// distinct bin of the wave (two rounds of ballot + broadcast) before the atomics, 61 us: the clustered keys do not serialise
// enough to pay for the election.  Letting the image's last workgroup find the threshold bin (a ticket behind a
// __threadfence(), to save the launches of sel_find_kernel): 573 us for the six launches of a step against 63 + 28 with the
// separate kernel -- a device-scope release in each of 5 000 workgroups costs far more than three small launches]
__global__ void __launch_bounds__(256) sel_hist_kernel(const uint32_t* __restrict__ keys, int64_t plane,
                                                       const uint32_t* __restrict__ state, uint32_t* __restrict__ hist,
                                                       int level, int shift, uint32_t binmask, uint32_t himask) {
  __shared__ uint32_t lh[SEL_BINS];
  const int n = blockIdx.y;
  if (level > 0 && state[SEL_STATE * n + 2] == 0) return;
  for (int i = threadIdx.x; i < SEL_BINS; i += 256) lh[i] = 0;
  __syncthreads();
  const uint32_t prefix = state[SEL_STATE * n];
  const uint32_t* kp = keys + (size_t)n * plane;
  const uint32_t sft = sel_shift_of(kp);
  const int64_t groups = (plane + sft + 3) >> 2;
  const int64_t gpb = (int64_t)SEL_HIST_CHUNKS * CHUNK / 4;        // groups per workgroup per round
  for (int64_t gb = (int64_t)blockIdx.x * gpb; gb < groups; gb += (int64_t)gridDim.x * gpb) {
#pragma unroll 1
    for (int j0 = 0; j0 < SEL_HIST_CHUNKS * 2; j0 += 4) {
      uint4 kv[4];
      uint32_t ok[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t g = gb + (int64_t)(j0 + u) * 256 + threadIdx.x;
        ok[u] = 0;
        kv[u] = make_uint4(0, 0, 0, 0);
        if (g < groups) kv[u] = sel_load4(kp, plane, sft, g, &ok[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t k4[4] = {kv[u].x, kv[u].y, kv[u].z, kv[u].w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (((ok[u] >> e) & 1u) && (k4[e] & himask) == prefix) atomicAdd(&lh[(k4[e] >> shift) & binmask], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SEL_BINS; i += 256) {
    const uint32_t c = lh[i];
    if (c) atomicAdd(&hist[(size_t)n * SEL_BINS + i], c);
  }
}

// one chunk per WAVE (64 lanes x 8 aligned groups of 4 keys, all eight loads in flight at once; no LDS, no barrier): masks,
// the chunk's counts (less | eq << 16) and, for an image that did not overflow, the candidates
__global__ void __launch_bounds__(256) sel_cand_kernel(const uint32_t* __restrict__ keys, int64_t plane,
                                                       uint32_t* __restrict__ state, uint32_t* __restrict__ blockcnt,
                                                       uint32_t* __restrict__ lessm, uint32_t* __restrict__ eqm,
                                                       uint32_t* __restrict__ cand, int nb) {
  const int n = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= nb) return;
  const uint32_t T = state[SEL_STATE * n];
  const bool over = state[SEL_STATE * n + 2] != 0;
  const uint32_t lowmask = over ? 0xffffffffu : ~((1u << SEL_SHIFT) - 1u);      // exact compare / digit compare
  const uint32_t* kp = keys + (size_t)n * plane;
  const uint32_t sft = sel_shift_of(kp);
  const int64_t groups = (plane + sft + 3) >> 2;
  uint32_t* cbuf = cand + (size_t)n * SEL_CAP * 2;
  constexpr int G = CHUNK / 256;                     // groups per lane
  uint4 kv[G];
  uint32_t ok[G];
#pragma unroll
  for (int j = 0; j < G; ++j) {
    const int64_t g = (int64_t)chunk * (CHUNK / 4) + j * 64 + lane;
    ok[j] = 0;
    kv[j] = make_uint4(0, 0, 0, 0);
    if (g < groups) kv[j] = sel_load4(kp, plane, sft, g, &ok[j]);
  }
  uint32_t cnt = 0;
#pragma unroll
  for (int j = 0; j < G; ++j) {
    const int64_t g = (int64_t)chunk * (CHUNK / 4) + j * 64 + lane;
    const uint32_t k4[4] = {kv[j].x, kv[j].y, kv[j].z, kv[j].w};
    uint32_t fl = 0, fe = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t d = k4[e] & lowmask;
      fl |= (uint32_t)(d < T) << e;
      fe |= (uint32_t)(d == T) << e;
    }
    fl &= ok[j];
    fe &= ok[j];
    cnt += (uint32_t)__popc(fl) | ((uint32_t)__popc(fe) << 16);
    if (!over && __ballot(fe != 0) != 0) {             // rare: the threshold bin holds at most SEL_CAP keys of the image
      const uint32_t c = (uint32_t)__popc(fe);
      const uint32_t inc = wave_incl_scan(c, lane);
      uint32_t base = 0;
      if (lane == 63) base = atomicAdd(&state[SEL_STATE * n + 3], inc);
      base = __shfl(base, 63);
      uint32_t slot = base + inc - c;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if ((fe >> e) & 1u) {
          if (slot < (uint32_t)SEL_CAP) { cbuf[2 * slot] = k4[e]; cbuf[2 * slot + 1] = (uint32_t)(4 * g + e); }
          ++slot;
        }
    }
    // eight lanes' nibbles make one mask word
    const int q = 4 * (lane & 7);
    uint32_t wl = fl << q, we = fe << q;
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) { wl |= __shfl_xor(wl, o); we |= __shfl_xor(we, o); }
    if ((lane & 7) == 0) {
      const size_t word = ((size_t)n * nb + chunk) * SEL_WORDS + j * 8 + (lane >> 3);
      lessm[word] = wl;
      eqm[word] = we;
    }
  }
  // chunk total: both 16-bit fields stay below 2^16 (CHUNK = 2048)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (lane == 0) blockcnt[(size_t)n * nb + chunk] = cnt;
}

// one workgroup per image: exact threshold from the candidates, masks and chunk counts corrected, chunk counts scanned
__global__ void __launch_bounds__(256) sel_resolve_kernel(uint32_t* __restrict__ state, uint32_t* __restrict__ blockcnt,
                                                          uint32_t* __restrict__ blockoff, uint32_t* __restrict__ lessm,
                                                          uint32_t* __restrict__ eqm, const uint32_t* __restrict__ cand,
                                                          int nb) {
  __shared__ uint32_t sh[8];
  __shared__ uint32_t below[SEL_SHIFT + 1];
  const int n = blockIdx.x;
  const int lane = threadIdx.x & 63;
  if (state[SEL_STATE * n + 2] == 0) {
    constexpr int PER = SEL_CAP / 256;
    const uint32_t ncand = min(state[SEL_STATE * n + 3], (uint32_t)SEL_CAP);
    const int per = (int)((ncand + 255u) / 256u);           // rounds of 256 candidates that hold any: a handful on real keys
    const uint32_t prefix = state[SEL_STATE * n], krem = state[SEL_STATE * n + 1];
    const uint32_t* cbuf = cand + (size_t)n * SEL_CAP * 2;
    uint32_t ck[PER], cv[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const uint32_t slot = j * 256 + threadIdx.x;
      ck[j] = slot < ncand ? cbuf[2 * slot] : 0xffffffffu;      // key and index in one round trip
      cv[j] = slot < ncand ? cbuf[2 * slot + 1] : 0u;
    }
    if (threadIdx.x <= SEL_SHIFT) below[threadIdx.x] = 0;
    __syncthreads();
    // T = the largest value with fewer than krem candidates below it = the krem-th smallest candidate
    uint32_t T = prefix;
    for (int bit = SEL_SHIFT - 1; bit >= -1; --bit) {
      const uint32_t trial = bit >= 0 ? (T | (1u << bit)) : T;      // last round: the count below T itself
      uint32_t c = 0;                                               // the wave's count: the same in every lane
#pragma unroll
      for (int j = 0; j < PER; ++j)
        if (j < per) c += (uint32_t)__popcll((unsigned long long)__ballot(ck[j] < trial));
      if (lane == 0 && c) atomicAdd(&below[bit + 1], c);
      __syncthreads();
      if (bit >= 0 && below[bit + 1] < krem) T = trial;
    }
    const uint32_t nbelow = below[0];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const uint32_t slot = j * 256 + threadIdx.x;
      if (slot < ncand && ck[j] != T) {
        const uint32_t v = cv[j];
        const size_t word = (size_t)n * nb * SEL_WORDS + (v >> 5);
        const uint32_t bitm = 1u << (v & 31u);
        atomicAnd(&eqm[word], ~bitm);
        uint32_t delta = 0u - (1u << 16);                 // one key fewer in the eq field
        if (ck[j] < T) { atomicOr(&lessm[word], bitm); delta += 1u; }
        atomicAdd(&blockcnt[(size_t)n * nb + v / CHUNK], delta);
      }
    }
    __syncthreads();                                       // every thread has read state and below[]
    if (threadIdx.x == 0) { state[SEL_STATE * n] = T; state[SEL_STATE * n + 1] = krem - nbelow; }
  }
  // the corrections above and the loads below are atomics on the same words, issued by threads of this workgroup on either
  // side of a barrier: no device-scope fence is needed (one here costs a write-back of the masks the pass before left in L2)
  __syncthreads();
  uint32_t carry_l = 0, carry_e = 0;
  for (int b0 = 0; b0 < nb; b0 += 256) {
    const int b = b0 + threadIdx.x;
    const uint32_t c = b < nb ? __hip_atomic_load(&blockcnt[(size_t)n * nb + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    uint32_t tl, te;
    const uint32_t el = block_excl_scan(c & 0xffffu, sh, &tl);
    const uint32_t ee = block_excl_scan(c >> 16, sh, &te);
    if (b < nb) {
      blockoff[((size_t)n * nb + b) * 2] = carry_l + el;
      blockoff[((size_t)n * nb + b) * 2 + 1] = carry_e + ee;
    }
    carry_l += tl;
    carry_e += te;
    __syncthreads();
  }
}

// the ordered write from the masks: one chunk per wave, one mask word (32 keys) per lane; compact_write_kernel's positions
__global__ void __launch_bounds__(256) sel_write_kernel(const uint32_t* __restrict__ keys, int64_t plane,
                                                        const uint32_t* __restrict__ state,
                                                        const uint32_t* __restrict__ blockoff,
                                                        const uint32_t* __restrict__ lessm, const uint32_t* __restrict__ eqm,
                                                        int nb, int k, int32_t* __restrict__ idx_out) {
  const int n = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= nb) return;
  const uint32_t krem = state[SEL_STATE * n + 1];
  const uint32_t nless = (uint32_t)k - krem;
  const int32_t sft = (int32_t)sel_shift_of(keys + (size_t)n * plane);
  const size_t word = ((size_t)n * nb + chunk) * SEL_WORDS + lane;
  uint32_t fl = lessm[word], fe = eqm[word];
  const uint32_t cl = (uint32_t)__popc(fl), ce = (uint32_t)__popc(fe);
  if (__ballot((cl | ce) != 0) == 0) return;
  uint32_t pl = wave_incl_scan(cl, lane) - cl + blockoff[((size_t)n * nb + chunk) * 2];
  uint32_t pe = wave_incl_scan(ce, lane) - ce + blockoff[((size_t)n * nb + chunk) * 2 + 1];
  const int32_t e0 = (int32_t)((int64_t)chunk * CHUNK + lane * 32) - sft;
  int32_t* o = idx_out + (size_t)n * k;
  while (fl) {
    const int j = __ffs((int)fl) - 1;
    fl &= fl - 1;
    if (pl < nless) o[pl] = e0 + j;
    ++pl;
  }
  while (fe && pe < krem) {
    const int j = __ffs((int)fe) - 1;
    fe &= fe - 1;
    o[nless + pe] = e0 + j;
    ++pe;
  }
}

__global__ void iota_kernel(int32_t* idx, int N, int k) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i < N * k) idx[i] = i % k;
}

// ---------------------------------------------------------------------------
// point sampling: half a wave per point, lane = 8 feature channels
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) point_features_kernel(const half_t* __restrict__ feat, int N, int fh, int fw,
                                                             int C, int feat_ld, const float* __restrict__ coarse,
                                                             int ncls, const int32_t* __restrict__ idx, int P, int H2,
                                                             int W2, half_t* __restrict__ x0, half_t* __restrict__ x1,
                                                             int ld) {
  const int hl = threadIdx.x & 31;
  const int64_t pt = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 5;
  if (pt >= (int64_t)N * P) return;
  const int n = (int)(pt / P);
  const int id = idx[pt];
  const int iy = id / W2, ix = id - iy * W2;
  const float sx = pr_sample_pos(ix, W2, fw), sy = pr_sample_pos(iy, H2, fh);      // common.h: no fma contraction
  const float fx0 = floorf(sx), fy0 = floorf(sy);
  const int xa = (int)fx0, ya = (int)fy0, xb = xa + 1, yb = ya + 1;
  const float lx = sx - fx0, ly = sy - fy0;
  const float w00 = (1.f - lx) * (1.f - ly), w01 = lx * (1.f - ly), w10 = (1.f - lx) * ly, w11 = lx * ly;
  const bool ok00 = xa >= 0 && xa < fw && ya >= 0 && ya < fh;
  const bool ok01 = xb >= 0 && xb < fw && ya >= 0 && ya < fh;
  const bool ok10 = xa >= 0 && xa < fw && yb >= 0 && yb < fh;
  const bool ok11 = xb >= 0 && xb < fw && yb >= 0 && yb < fh;
  const int CG = C >> 3;
  half_t* r0 = x0 + (size_t)pt * ld;
  half_t* r1 = x1 + (size_t)pt * ld;
  const half_t* fb = feat + (size_t)n * fh * fw * feat_ld;
  for (int cg = hl; cg < CG; cg += 32) {
    float a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto accum = [&](bool ok, int yy, int xx, float wt) {
      if (ok) {
        f16x8 v = *reinterpret_cast<const f16x8*>(fb + ((size_t)yy * fw + xx) * feat_ld + cg * 8);
#pragma unroll
        for (int c = 0; c < 8; ++c) a[c] = fmaf((float)v[c], wt, a[c]);
      }
    };
    accum(ok00, ya, xa, w00);
    accum(ok01, ya, xb, w01);
    accum(ok10, yb, xa, w10);
    accum(ok11, yb, xb, w11);
    f16x8 o;
#pragma unroll
    for (int c = 0; c < 8; ++c) o[c] = (half_t)a[c];
    *reinterpret_cast<f16x8*>(r0 + cg * 8) = o;
  }
  // tail chunks [C, ld): coarse logits in the first ncls slots, zeros elsewhere
  const int tail = (ld - C) >> 3;
  if (hl < tail) {
    f16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hl == 0) {
      for (int c = 0; c < ncls && c < 8; ++c) {
        const float* cb = coarse + ((size_t)n * ncls + c) * fh * fw;
        float v = 0.f;
        if (ok00) v = fmaf(cb[ya * fw + xa], w00, v);
        if (ok01) v = fmaf(cb[ya * fw + xb], w01, v);
        if (ok10) v = fmaf(cb[yb * fw + xa], w10, v);
        if (ok11) v = fmaf(cb[yb * fw + xb], w11, v);
        o[c] = (half_t)v;
      }
    }
    *reinterpret_cast<f16x8*>(r0 + C + hl * 8) = o;
    *reinterpret_cast<f16x8*>(r1 + C + hl * 8) = o;
  }
}

// ---------------------------------------------------------------------------
// Fused point head (point_rend.py:181-188,241-269, eval): point sampling -> num_fc x (Conv1d k=1 + ReLU, coarse logits
// concatenated at every layer) -> predictor -> scatter, for a tile of 256 points per workgroup.  Replaces
// point_features_kernel + num_fc implicit-GEMM launches + head1x1_kernel: the (points x 320) rows never reach HBM.
//   LDS: X[256 points][LD channels] fp16 (all 160 KiB at LD = 320), rows of LD*2 bytes, 16-byte chunk c of each 128-byte segment stored at
//        c ^ (row & 7) (conflict-free ds_read_b128 fragment reads, as in conv_igemm.hip).
//   gather    : half a wave per point, lane = 8 channels; arithmetic of point_features_kernel (fmaf chain per tap).
//   layer     : wave w owns couts [MT*16*w, +MT*16) x all 256 points; K walked in ascending 32-channel steps from a zero
//               accumulator (the order of conv_igemm_kernel: results are bit-identical to the unfused launches); the
//               wave's weight fragments of the WHOLE layer (MT x LD/32 x 4 VGPRs) are loaded from L2 in one burst,
//               the next layer's during this layer's epilogue, so the K loop waits for LDS only [first version:
//               fragments fetched per K-step at two workgroups per CU -- 302 us per launch, 8x its MFMA time, every
//               K-step exposed an L2 round trip]; bias + ReLU + ONE fp16 rounding, written back over X[:, 0:C) after
//               a barrier.  Two passes of 128 points per layer (64 accumulator VGPRs beside 72 weight VGPRs).
//   Measured (32 x 8192 points, MI355X): 257 us per launch = gather 88 (0.54 GB of scattered 512-byte pixel rows: at the
//   memory system's rate) + layers ~115 (MFMA time 60) + predictor ~40, against 120 + 330 + 55 us for the launches it
//   replaces; bit-identical sem_logits (tests/test_gpu_model.py).
//   predictor : half a wave per point on the fp16 row, fp32 weights, the reduction order of head1x1_kernel.
template <int C>
struct PrCfg {
  static constexpr int MT = C / 128;          // 16-cout tiles per wave (8 waves cover C couts)
};

struct PrParams {
  const half_t* feat; int N, fh, fw, feat_ld;
  const float* coarse; int ncls;
  const int32_t* idx; int P, H2, W2;
  const half_t* w[4]; const float* b[4]; int num_fc;    // fc layers: [C][LD] fp16, bias fp32
  const float* pw; const float* pb;                     // predictor [ncls][LD] fp32
  float* out; int64_t plane;
  int64_t npts; int tiles;
};

template <int C, int LD>
__global__ void __launch_bounds__(512, 1) pr_mlp_kernel(const PrParams p) {
  constexpr int MT = PrCfg<C>::MT;
  constexpr int LDB = LD * 2;                 // bytes per row
  // K-steps: channels [C + 8, LD) of a row are zeros (ncls <= 8) and so are the weights' pad columns, so the steps beyond
  // C/32 + 1 add exact zeros: skipping them leaves every sum bit-identical
  constexpr int KSTEPS = C / 32 + 1;
  constexpr int KC = LD / 8;                  // 16-byte chunks per row
  constexpr int PT = 256, QT = PT / 16;       // points per tile, 16-point MFMA tiles
  extern __shared__ __attribute__((aligned(1024))) char X[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hl = lane & 31, hw = tid >> 5;    // half-wave index 0..15
  const int fr = lane & 15, fq = lane >> 4;
  auto xoff = [](int row, int chunk) { return row * LDB + (chunk >> 3) * 128 + (((chunk & 7) ^ (row & 7)) << 4); };

  for (int tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const int64_t g0 = (int64_t)tile * PT;
    // ---------------- gather ----------------
    // 16 points per half-wave, four at a time: the sixteen 16-byte feature taps of a group (and lane 0's coarse-logit
    // taps) are in flight before the first is used.  [measured: this phase moves 0.54 GB of scattered 512-byte pixel
    // rows per launch in ~105 us = 5 TB/s -- it is at the memory system's rate, deeper batching (8 points) was slower]
    auto sample_geometry = [&](int row, int& n, int& xa, int& ya, float* wt, bool* ok) {
      const int64_t pt = g0 + row;
      const bool live = pt < p.npts;
      const int id = live ? p.idx[pt] : 0;
      n = live ? (int)(pt / p.P) : 0;
      const int iy = id / p.W2, ix = id - iy * p.W2;
      const float sx = pr_sample_pos(ix, p.W2, p.fw), sy = pr_sample_pos(iy, p.H2, p.fh);      // common.h: no fma contraction
      const float fx0 = floorf(sx), fy0 = floorf(sy);
      xa = (int)fx0; ya = (int)fy0;
      const int xb = xa + 1, yb = ya + 1;
      const float lx = sx - fx0, ly = sy - fy0;
      wt[0] = (1.f - lx) * (1.f - ly); wt[1] = lx * (1.f - ly); wt[2] = (1.f - lx) * ly; wt[3] = lx * ly;
      ok[0] = live && xa >= 0 && xa < p.fw && ya >= 0 && ya < p.fh;
      ok[1] = live && xb >= 0 && xb < p.fw && ya >= 0 && ya < p.fh;
      ok[2] = live && xa >= 0 && xa < p.fw && yb >= 0 && yb < p.fh;
      ok[3] = live && xb >= 0 && xb < p.fw && yb >= 0 && yb < p.fh;
    };
    {
      constexpr int GB = 4;
#pragma unroll 1
      for (int j0 = 0; j0 < PT / 16; j0 += GB) {
        int nn[GB], xa[GB], ya[GB];
        float wt[GB][4];
        bool ok[GB][4];
#pragma unroll
        for (int u = 0; u < GB; ++u) sample_geometry(hw + 16 * (j0 + u), nn[u], xa[u], ya[u], wt[u], ok[u]);
        if (hl < C / 8) {
          f16x8 v[GB][4];
#pragma unroll
          for (int u = 0; u < GB; ++u) {
            const half_t* fb = p.feat + (size_t)nn[u] * p.fh * p.fw * p.feat_ld + hl * 8;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              const int yy = ya[u] + (t >> 1), xx = xa[u] + (t & 1);
              const half_t* src = ok[u][t] ? fb + ((size_t)yy * p.fw + xx) * p.feat_ld : p.feat;
              v[u][t] = *reinterpret_cast<const f16x8*>(src);
            }
          }
#pragma unroll
          for (int u = 0; u < GB; ++u) {
            float a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int t = 0; t < 4; ++t)
              if (ok[u][t]) {
#pragma unroll
                for (int c = 0; c < 8; ++c) a[c] = fmaf((float)v[u][t][c], wt[u][t], a[c]);
              }
            f16x8 o;
#pragma unroll
            for (int c = 0; c < 8; ++c) o[c] = (half_t)a[c];
            *reinterpret_cast<f16x8*>(X + xoff(hw + 16 * (j0 + u), hl)) = o;
          }
        }
        // tail chunks [C, LD): coarse logits in the first ncls slots, zeros elsewhere
        if (hl < (LD - C) / 8) {
          f16x8 o[GB];
#pragma unroll
          for (int u = 0; u < GB; ++u) o[u] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
          if (hl == 0) {
            for (int c = 0; c < p.ncls && c < 8; ++c) {
              float cv[GB][4];
#pragma unroll
              for (int u = 0; u < GB; ++u) {
                const float* cb = p.coarse + ((size_t)nn[u] * p.ncls + c) * p.fh * p.fw;
#pragma unroll
                for (int t = 0; t < 4; ++t)
                  cv[u][t] = ok[u][t] ? cb[(ya[u] + (t >> 1)) * p.fw + xa[u] + (t & 1)] : 0.f;
              }
#pragma unroll
              for (int u = 0; u < GB; ++u) {
                float vv = 0.f;
#pragma unroll
                for (int t = 0; t < 4; ++t)
                  if (ok[u][t]) vv = fmaf(cv[u][t], wt[u][t], vv);
#pragma unroll
                for (int e = 0; e < 8; ++e) o[u][e] = (e == c) ? (half_t)vv : o[u][e];     // runtime c: select, no dynamic index
              }
            }
          }
#pragma unroll
          for (int u = 0; u < GB; ++u) *reinterpret_cast<f16x8*>(X + xoff(hw + 16 * (j0 + u), C / 8 + hl)) = o[u];
        }
      }
    }
    __syncthreads();
    // ---------------- fc layers ----------------
    f16x8 wf[KSTEPS][MT];
    auto load_weights = [&](int f) {
      const half_t* wb = p.w[f] + (size_t)(wave * MT * 16 + fr) * LD + fq * 8;
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks)
#pragma unroll
        for (int c = 0; c < MT; ++c) wf[ks][c] = *reinterpret_cast<const f16x8*>(wb + (size_t)c * 16 * LD + ks * 32);
    };
    load_weights(0);
    for (int f = 0; f < p.num_fc; ++f) {
      // two passes of 128 points (64 accumulator VGPRs beside the layer's 80 weight VGPRs): a pass's rows are rewritten
      // with the layer's output as soon as every wave has finished reading them
#pragma unroll 1
      for (int hf = 0; hf < PT / 128; ++hf) {
        f32x4 acc[MT][8];
#pragma unroll
        for (int c = 0; c < MT; ++c)
#pragma unroll
          for (int q = 0; q < 8; ++q) acc[c][q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const f16x8 pf = *reinterpret_cast<const f16x8*>(X + xoff(hf * 128 + q * 16 + fr, ks * 4 + fq));
#pragma unroll
            for (int c = 0; c < MT; ++c) acc[c][q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[ks][c], pf, acc[c][q], 0, 0, 0);
          }
        }
        if (hf + 1 == PT / 128 && f + 1 < p.num_fc) load_weights(f + 1);      // in flight during the barrier and the epilogue
        __syncthreads();      // every wave is done reading these rows
#pragma unroll
        for (int c = 0; c < MT; ++c) {
          const int co = wave * MT * 16 + c * 16 + fq * 4;       // 4 consecutive couts of this lane
          const float4 bv = *reinterpret_cast<const float4*>(p.b[f] + co);
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int row = hf * 128 + q * 16 + fr;
            f16x4 o;
            o[0] = (half_t)fmaxf(acc[c][q][0] + bv.x, 0.f);
            o[1] = (half_t)fmaxf(acc[c][q][1] + bv.y, 0.f);
            o[2] = (half_t)fmaxf(acc[c][q][2] + bv.z, 0.f);
            o[3] = (half_t)fmaxf(acc[c][q][3] + bv.w, 0.f);
            *reinterpret_cast<f16x4*>(X + xoff(row, co >> 3) + (co & 7) * 2) = o;
          }
        }
      }
      __syncthreads();
    }
    // ---------------- predictor + scatter ----------------
    // class by class: the class's fp32 weights (two 8-channel chunks per lane) are loaded once, then the half-wave walks
    // its 16 rows; per row the arithmetic and the reduction order of head1x1_kernel
    for (int c = 0; c < p.ncls; ++c) {
      float wv[2][8];
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int kc = hl + 32 * jj;
        if (kc < KC) {
          const float4* wp = reinterpret_cast<const float4*>(p.pw + (size_t)c * LD + kc * 8);
          const float4 w0 = wp[0], w1 = wp[1];
          wv[jj][0] = w0.x; wv[jj][1] = w0.y; wv[jj][2] = w0.z; wv[jj][3] = w0.w;
          wv[jj][4] = w1.x; wv[jj][5] = w1.y; wv[jj][6] = w1.z; wv[jj][7] = w1.w;
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) wv[jj][e] = 0.f;
        }
      }
      const float bias = p.pb[c];
#pragma unroll 4
      for (int j = 0; j < PT / 16; ++j) {
        const int row = hw + 16 * j;
        const int64_t pt = g0 + row;
        const bool live = pt < p.npts;
        float sacc = 0.f;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          const int kc = hl + 32 * jj;
          if (kc < KC) {
            const f16x8 v = *reinterpret_cast<const f16x8*>(X + xoff(row, kc));
#pragma unroll
            for (int e = 0; e < 8; ++e) sacc = fmaf((float)v[e], wv[jj][e], sacc);
          }
        }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) sacc += __shfl_xor(sacc, o);
        if (hl == 0 && live) {
          const int n = (int)(pt / p.P);
          p.out[((size_t)n * p.ncls + c) * p.plane + (int64_t)p.idx[pt]] = sacc + bias;
        }
      }
    }
    __syncthreads();        // X is rewritten by the next tile's gather
  }
}

inline int grid_for(int64_t total, int per_block = 256, int cap = 256 * 16) {
  int64_t g = (total + per_block - 1) / per_block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace

int launch_upsample2x_keys(const float* in, int N, int C, int h, int w, float* out, uint32_t* keys, hipStream_t s) {
  int64_t total = (int64_t)N * 4 * h * w;
  const char* legacy_env = getenv("EMP_PR_UP2X_LEGACY");      // =1: one output per thread (read per call: A/B; identical output)
  if ((legacy_env && legacy_env[0] == '1') || total >= (1ll << 31)) {
    hipLaunchKernelGGL(upsample2x_keys_kernel, dim3(grid_for(total)), dim3(256), 0, s, in, N, C, h, w, out, keys, total);
    EMP_LAUNCH_CHECK();
    return EMP_OK;
  }
  const int W = 2 * w, Wq = (W + 3) / 4;
  const int groups = N * 2 * h * Wq;                          // <= total
  const uintptr_t bases = (uintptr_t)out | (uintptr_t)keys;
  const int vec = (W % 4 == 0 && bases % 16 == 0) ? 4 : (bases % 8 == 0 ? 2 : 1);
  auto kern = vec == 4 ? upsample2x_keys4_kernel<4> : vec == 2 ? upsample2x_keys4_kernel<2> : upsample2x_keys4_kernel<1>;
  hipLaunchKernelGGL(kern, dim3(cdiv(groups, 256)), dim3(256), 0, s, in, C, h, w, out, keys, Wq, groups);
  EMP_LAUNCH_CHECK();
  return EMP_OK;
}

static inline int sel_chunks(int64_t plane) { return (int)cdiv64(plane + 3, CHUNK); }      // + 3: the alignment shift

size_t topk_work_bytes(int N, int64_t plane) {
  // hist | state | chunk counts | chunk offsets (2) | less mask | eq mask | candidates (key, index); the legacy select
  // lays its smaller arrays over the start of the same buffer
  const size_t nb = (size_t)sel_chunks(plane);
  return (size_t)N * (SEL_BINS + SEL_STATE + nb * 3 + nb * SEL_WORDS * 2 + (size_t)SEL_CAP * 2) * sizeof(uint32_t) + 256;
}

static int launch_topk_legacy(const uint32_t* keys, int N, int64_t plane, int k, void* work, int32_t* idx_out,
                              hipStream_t s) {
  const int nb = (int)cdiv64(plane, CHUNK);
  uint32_t* hist = (uint32_t*)work;
  uint32_t* state = hist + (size_t)N * 256;
  uint32_t* blockcnt = state + (size_t)N * 4;
  uint32_t* blockoff = blockcnt + (size_t)N * nb;
  hipLaunchKernelGGL(init_state_kernel, dim3(cdiv(N * 256, 256)), dim3(256), 0, s, state, hist, N, (uint32_t)k);
  EMP_LAUNCH_CHECK();
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const uint32_t himask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    hipLaunchKernelGGL(radix_hist_kernel, dim3(nb, N), dim3(256), 0, s, keys, plane, state, hist, shift, himask);
    EMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(radix_select_kernel, dim3(N), dim3(256), 0, s, hist, state, shift);
    EMP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(compact_count_kernel, dim3(nb, N), dim3(256), 0, s, keys, plane, state, blockcnt, nb);
  EMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(compact_scan_kernel, dim3(N), dim3(256), 0, s, blockcnt, blockoff, nb);
  EMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(compact_write_kernel, dim3(nb, N), dim3(256), 0, s, keys, plane, state, blockoff, nb, k, idx_out);
  EMP_LAUNCH_CHECK();
  return EMP_OK;
}

// keys: (N, plane) non-negative-float bit patterns; selects the k smallest per image.
int launch_topk_smallest(const uint32_t* keys, int N, int64_t plane, int k, void* work, size_t work_bytes,
                         int32_t* idx_out, hipStream_t s) {
  EMP_REQUIRE(k > 0 && plane > 0, "topk: k=%d plane=%lld", k, (long long)plane);
  if ((int64_t)k >= plane) {
    EMP_REQUIRE((int64_t)k == plane, "topk: k > plane");
    hipLaunchKernelGGL(iota_kernel, dim3(cdiv(N * k, 256)), dim3(256), 0, s, idx_out, N, k);
    EMP_LAUNCH_CHECK();
    return EMP_OK;
  }
  EMP_REQUIRE(work_bytes >= topk_work_bytes(N, plane), "topk: workspace too small");
  const char* legacy_env = getenv("EMP_TOPK_LEGACY");      // =1: the four-pass radix select (read per call: A/B; identical output)
  if (legacy_env && legacy_env[0] == '1') return launch_topk_legacy(keys, N, plane, k, work, idx_out, s);
  const int nb = sel_chunks(plane);
  uint32_t* hist = (uint32_t*)work;
  uint32_t* state = hist + (size_t)N * SEL_BINS;
  uint32_t* blockcnt = state + (size_t)N * SEL_STATE;
  uint32_t* blockoff = blockcnt + (size_t)N * nb;
  uint32_t* lessm = blockoff + (size_t)N * nb * 2;
  uint32_t* eqm = lessm + (size_t)N * nb * SEL_WORDS;
  uint32_t* cand = eqm + (size_t)N * nb * SEL_WORDS;
  hipLaunchKernelGGL(sel_init_kernel, dim3(cdiv(N * SEL_BINS, 256)), dim3(256), 0, s, state, hist, N, (uint32_t)k);
  EMP_LAUNCH_CHECK();
  const int hb = (int)cdiv64(plane + 3, (int64_t)SEL_HIST_CHUNKS * CHUNK);
  // level 0 for every image; levels 1 and 2 return at once unless the image's threshold bin overflowed the candidate
  // buffer, so their grids are capped (the workgroups of an overflow image walk it in rounds)
  const int lv_shift[3] = {SEL_SHIFT, SEL_L2_SHIFT, 0};
  const uint32_t lv_bins[3] = {(uint32_t)SEL_BINS - 1u, (1u << SEL_L2_BITS) - 1u, (1u << SEL_L2_SHIFT) - 1u};
  const uint32_t lv_hi[3] = {0u, 0xffffffffu << SEL_SHIFT, 0xffffffffu << SEL_L2_SHIFT};
  for (int level = 0; level < 3; ++level) {
    const int gx = level == 0 ? hb : (hb < 64 ? hb : 64);
    hipLaunchKernelGGL(sel_hist_kernel, dim3(gx, N), dim3(256), 0, s, keys, plane, state, hist, level, lv_shift[level],
                       lv_bins[level], lv_hi[level]);
    EMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(sel_find_kernel, dim3(N), dim3(256), 0, s, hist, state, level, lv_shift[level]);
    EMP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(sel_cand_kernel, dim3(cdiv(nb, 4), N), dim3(256), 0, s, keys, plane, state, blockcnt, lessm, eqm, cand, nb);
  EMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(sel_resolve_kernel, dim3(N), dim3(256), 0, s, state, blockcnt, blockoff, lessm, eqm, cand, nb);
  EMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(sel_write_kernel, dim3(cdiv(nb, 4), N), dim3(256), 0, s, keys, plane, state, blockoff, lessm, eqm, nb, k,
                     idx_out);
  EMP_LAUNCH_CHECK();
  return EMP_OK;
}

int launch_point_features(const half_t* feat, int N, int fh, int fw, int C, int feat_ld, const float* coarse, int ncls,
                          const int32_t* idx, int P, int H2, int W2, half_t* x0, half_t* x1, int ld, hipStream_t s) {
  EMP_REQUIRE(C % 8 == 0 && ld % 8 == 0 && ld >= C + 8 && ncls <= 8, "point_features: bad channel layout");
  EMP_REQUIRE((ld - C) / 8 <= 32, "point_features: tail too wide");
  int64_t pts = (int64_t)N * P;
  hipLaunchKernelGGL(point_features_kernel, dim3((unsigned)cdiv64(pts, 8)), dim3(256), 0, s, feat, N, fh, fw, C, feat_ld,
                     coarse, ncls, idx, P, H2, W2, x0, x1, ld);
  EMP_LAUNCH_CHECK();
  return EMP_OK;
}

bool pr_mlp_supported(int C, int ld, int ncls, int num_fc) {
  return ((C == 256 && ld == 320) || (C == 128 && ld == 192)) && ncls >= 1 && ncls <= 8 && num_fc >= 1 && num_fc <= 4;
}

int launch_pr_mlp(const half_t* feat, int N, int fh, int fw, int C, int feat_ld, const float* coarse, int ncls,
                  const int32_t* idx, int P, int H2, int W2, const half_t* const* fc_w, const float* const* fc_b,
                  int num_fc, int ld, const float* pred_w, const float* pred_b, float* out, int64_t plane,
                  hipStream_t s) {
  EMP_REQUIRE(pr_mlp_supported(C, ld, ncls, num_fc), "pr_mlp: unsupported shape C=%d ld=%d", C, ld);
  PrParams p{};
  p.feat = feat; p.N = N; p.fh = fh; p.fw = fw; p.feat_ld = feat_ld;
  p.coarse = coarse; p.ncls = ncls; p.idx = idx; p.P = P; p.H2 = H2; p.W2 = W2;
  for (int i = 0; i < num_fc; ++i) { p.w[i] = fc_w[i]; p.b[i] = fc_b[i]; }
  p.num_fc = num_fc; p.pw = pred_w; p.pb = pred_b; p.out = out; p.plane = plane;
  p.npts = (int64_t)N * P;
  p.tiles = (int)cdiv64(p.npts, 256);
  const int grid = p.tiles < 256 ? p.tiles : 256;       // one workgroup per CU
  const size_t lds = (size_t)256 * ld * 2;
  if (C == 256) {
    if (int rc = ensure_dyn_lds(reinterpret_cast<const void*>(&pr_mlp_kernel<256, 320>), (int)lds)) return rc;
    hipLaunchKernelGGL((pr_mlp_kernel<256, 320>), dim3(grid), dim3(512), lds, s, p);
  } else {
    if (int rc = ensure_dyn_lds(reinterpret_cast<const void*>(&pr_mlp_kernel<128, 192>), (int)lds)) return rc;
    hipLaunchKernelGGL((pr_mlp_kernel<128, 192>), dim3(grid), dim3(512), lds, s, p);
  }
  EMP_LAUNCH_CHECK();
  return EMP_OK;
}

}  // namespace emp
