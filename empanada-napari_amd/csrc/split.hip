// Split Labels on the device (empanada_napari/_merge_split_widget.py:422-634): the parts of one turn that are parallel work.
//   per label (:517-547):  shed_box = the label's TIGHT box (no padding, :519); binary = crop == label (:520)
//   distance mode (:428-447):  distance = ndi.distance_transform_edt(binary); coords = peak_local_max(distance, min_distance);
//                              markers = ndi.label(marker mask); energy = -distance
//   points mode (:449-456):    markers = ndi.label(the points); energy = binary (one plateau)
//   both (:527-545):           new = watershed(energy, markers, mask=binary); labels[box][binary] = new[binary] + max_label
// Only voxels of the label itself are rewritten: the turns of a call touch disjoint voxels and are batched here as BOXES.  The
// id bookkeeping (:533-545), the greedy spacing of the peaks and ndi.label of the few survivors stay on the host (labels.py).
//
// A box is 8 int64 {z0, y0, x0, nz, ny, nx, offset, label}; an image is nz = 1.  Every per-voxel array (d2, the work arrays, the
// markers) holds a box at [offset, offset + nz ny nx) in the box's own raster order, so the arrays are as large as the boxes, not
// as the array.  The entries take the boxes from the HOST, check them against the array and the capacity, and upload them.
//
//   emp_split_edt     the exact squared Euclidean distance to the nearest voxel OF THE CROP that is not the label (outside the
//                     crop is not background), int32.  split_rows_kernel: one wave per row, the nearest background to the left
//                     and to the right from ballots; split_env_kernel: per remaining axis the lower envelope of the parabolas
//                     f(j) + (u - j)^2 (Meijster et al. 2000, integer Sep), one thread per line, neighbouring threads on
//                     neighbouring x.  A row / line without background carries EMP_SPLIT_INF = 2^30: a box must have
//                     nz^2 + ny^2 + nx^2 < 2^30, so every true distance is below the sentinel and sentinel + (u - j)^2 < 2^31.
//                     Pinned against scipy.ndimage.distance_transform_edt, exactly.
//   emp_split_peaks   peak_local_max's candidates: d2 == maximum_filter(d2, size 2d + 1, mode='nearest') (separable, one pass
//                     per axis, clamped to the box), d2 > min(d2), not within d of a face of an axis longer than 1 (size-1 axes
//                     are squeezed, :434-440), compacted in raster order, box after box.  "Every voxel is a maximum -> none" needs
//                     no pass of its own: neighbouring voxels that differ cannot both be maxima, so it only happens on a constant
//                     image, where d2 > min fails everywhere.  The filter is pinned against scipy; the predicate is skimage's
//                     restated from memory and NOT pinned.
//   emp_split_flood   the level-synchronous form of the watershed (see empanada_hip.h): every mask voxel recomputes its time
//                     (L, g) and label from its face neighbours' CURRENT values, double-buffered (a sweep reads one buffer and
//                     writes the other, so the number of sweeps is reproducible), until a sweep changes nothing.  No atomic
//                     minimum: a stale label with an equal time would stick.
//   emp_split_write   vol[box][vol == label] = base + marker
#include <algorithm>
#include <vector>

#include "common.h"

namespace emp {
namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_WAVES = SP_THREADS / 64;
constexpr int SP_CHUNK = 4 * SP_THREADS;      // voxels per block of the candidate compaction
constexpr int32_t SP_INF = EMP_SPLIT_INF;
constexpr int SP_MAX_BOXES = 65535;           // grid.y
constexpr int SP_BATCH = 8;                   // sweeps between two looks at the change flags
constexpr int32_t SP_MARK = 0x40000000;       // in a flood label: the voxel is a marker
constexpr int32_t SP_ID = 0x3fffffff;
constexpr uint64_t SP_NEVER = ~0ull;

struct SpBox {
  int z0, y0, x0, nz, ny, nx;
  int64_t off;
  uint64_t label;
  __host__ __device__ int64_t voxels() const { return (int64_t)nz * ny * nx; }
};

__host__ __device__ inline SpBox sp_box(const int64_t* b) {
  SpBox o;
  o.z0 = (int)b[0];
  o.y0 = (int)b[1];
  o.x0 = (int)b[2];
  o.nz = (int)b[3];
  o.ny = (int)b[4];
  o.nx = (int)b[5];
  o.off = b[6];
  o.label = (uint64_t)b[7];
  return o;
}

template <int S> struct SpElem;
template <> struct SpElem<1> { typedef uint8_t type; };
template <> struct SpElem<2> { typedef uint16_t type; };
template <> struct SpElem<4> { typedef uint32_t type; };
template <> struct SpElem<8> { typedef uint64_t type; };

// ---------------------------------------------------------------------------
// squared distance along the rows
// ---------------------------------------------------------------------------
// One wave per row (z, y) of a box.  Forward over the row in words of 64 voxels: the nearest background at or left of a voxel is
// the highest set bit at or below its lane, or the last one of the words before; then the same backward for the right side.
template <int S>
__global__ void __launch_bounds__(SP_THREADS) split_rows_kernel(const void* __restrict__ vol, int H, int W, const int64_t* __restrict__ boxes,
                                                                int32_t* __restrict__ out) {
  typedef typename SpElem<S>::type T;
  const SpBox b = sp_box(boxes + 8 * blockIdx.y);
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * SP_WAVES + (threadIdx.x >> 6);
  if (row >= (int64_t)b.nz * b.ny) return;      // uniform over the wave
  const int z = (int)(row / b.ny), y = (int)(row % b.ny);
  const T* src = (const T*)vol + ((int64_t)(b.z0 + z) * H + b.y0 + y) * W + b.x0;
  int32_t* dst = out + b.off + row * b.nx;
  const T label = (T)b.label;
  const uint64_t upto = lane == 63 ? ~0ull : ((2ull << lane) - 1);      // the lanes at or below this one
  const uint64_t from = ~0ull << lane;
  int last = -1;
  for (int c0 = 0; c0 < b.nx; c0 += 64) {
    const int x = c0 + lane;
    const uint64_t word = __ballot(x < b.nx && src[x] != label);
    const uint64_t m = word & upto;
    const int near = m ? c0 + 63 - __clzll((long long)m) : last;
    if (x < b.nx) dst[x] = near < 0 ? 0x7fffffff : x - near;
    if (word) last = c0 + 63 - __clzll((long long)word);
  }
  last = -1;
  for (int c0 = ((b.nx - 1) / 64) * 64; c0 >= 0; c0 -= 64) {
    const int x = c0 + lane;
    const uint64_t word = __ballot(x < b.nx && src[x] != label);
    const uint64_t m = word & from;
    const int near = m ? c0 + __ffsll((unsigned long long)m) - 1 : last;
    if (x < b.nx) {
      const int left = dst[x];
      const int right = near < 0 ? 0x7fffffff : near - x;
      const int d = left < right ? left : right;
      dst[x] = d == 0x7fffffff ? SP_INF : d * d;      // d < nx, nx^2 < 2^30
    }
    if (word) last = c0 + __ffsll((unsigned long long)word) - 1;
  }
}

// ---------------------------------------------------------------------------
// lower envelope of parabolas along y (axis 1) or z (axis 0)
// ---------------------------------------------------------------------------
// out[u] = min_j in[j] + (u - j)^2 along a line, clamped to the sentinel.  One thread per line; element k of a line and slot k of
// its two stacks (s: the parabola, t: from where it is the lowest) sit at the same place of their arrays, so threads on
// neighbouring x read and write neighbouring words.  Meijster's scan: all integers, Sep is a floor division of a numerator that
// the loop before it has made non-negative.
__global__ void __launch_bounds__(SP_THREADS) split_env_kernel(const int64_t* __restrict__ boxes, int axis, const int32_t* __restrict__ in,
                                                               int32_t* __restrict__ out, int32_t* __restrict__ s, int32_t* __restrict__ t) {
  const SpBox b = sp_box(boxes + 8 * blockIdx.y);
  const int m = axis == 1 ? b.ny : b.nz;
  const int64_t lines = b.voxels() / m;
  const int64_t l = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (l >= lines) return;
  int64_t base, stride;
  if (axis == 1) {
    base = b.off + (l / b.nx) * (int64_t)b.ny * b.nx + l % b.nx;
    stride = b.nx;
  } else {
    base = b.off + l;
    stride = (int64_t)b.ny * b.nx;
  }
  const int32_t* f = in + base;
  int32_t* o = out + base;
  if (m == 1) {
    o[0] = f[0];
    return;
  }
  int32_t* ss = s + base;
  int32_t* tt = t + base;
  int q = 0;
  ss[0] = 0;
  tt[0] = 0;
  int sq = 0, tq = 0;              // the top of the stack, kept in registers
  int64_t fq = f[0];               // f at the top's parabola
  for (int u = 1; u < m; ++u) {
    const int64_t fu = f[(int64_t)u * stride];
    while (q >= 0) {
      const int64_t a = (int64_t)(tq - sq) * (tq - sq) + fq, c = (int64_t)(tq - u) * (tq - u) + fu;
      if (a <= c) break;
      --q;
      if (q >= 0) {
        sq = ss[(int64_t)q * stride];
        tq = tt[(int64_t)q * stride];
        fq = f[(int64_t)sq * stride];
      }
    }
    if (q < 0) {
      q = 0;
      sq = u;
      tq = 0;
      fq = fu;
      ss[0] = u;
    } else {
      const int64_t w = 1 + ((int64_t)u * u - (int64_t)sq * sq + fu - fq) / (2 * (int64_t)(u - sq));
      if (w < m) {
        ++q;
        sq = u;
        tq = (int)w;
        fq = fu;
        ss[(int64_t)q * stride] = u;
        tt[(int64_t)q * stride] = (int)w;
      }
    }
  }
  for (int u = m - 1; u >= 0; --u) {
    const int64_t v = (int64_t)(u - sq) * (u - sq) + fq;
    o[(int64_t)u * stride] = v < SP_INF ? (int32_t)v : SP_INF;
    if (u == tq && q > 0) {
      --q;
      sq = ss[(int64_t)q * stride];
      tq = tt[(int64_t)q * stride];
      fq = f[(int64_t)sq * stride];
    }
  }
}

// ---------------------------------------------------------------------------
// peak candidates
// ---------------------------------------------------------------------------
struct SpPos {
  int64_t p;
  int z, y, x;
};

__device__ __forceinline__ bool sp_pos(const SpBox& b, int64_t p, SpPos& o) {
  if (p >= b.voxels()) return false;
  o.p = p;
  o.x = (int)(p % b.nx);
  o.y = (int)((p / b.nx) % b.ny);
  o.z = (int)(p / ((int64_t)b.nx * b.ny));
  return true;
}

// the running maximum along one axis (2: x, 1: y, 0: z), window 2 d + 1 clamped to the box; with `mins` also the box's minimum
__global__ void __launch_bounds__(SP_THREADS) split_max_kernel(const int64_t* __restrict__ boxes, int axis, int d, const int32_t* __restrict__ in,
                                                               int32_t* __restrict__ out, int32_t* __restrict__ mins) {
  const SpBox b = sp_box(boxes + 8 * blockIdx.y);
  SpPos q;
  const bool live = sp_pos(b, (int64_t)blockIdx.x * SP_THREADS + threadIdx.x, q);
  int32_t own = 0x7fffffff;
  if (live) {
    const int c = axis == 2 ? q.x : axis == 1 ? q.y : q.z;
    const int n = axis == 2 ? b.nx : axis == 1 ? b.ny : b.nz;
    const int64_t stride = axis == 2 ? 1 : axis == 1 ? b.nx : (int64_t)b.nx * b.ny;
    const int lo = c - d < 0 ? 0 : c - d, hi = c + d > n - 1 ? n - 1 : c + d;
    const int32_t* f = in + b.off + q.p - (int64_t)c * stride;
    own = f[(int64_t)c * stride];
    int32_t best = own;
    for (int k = lo; k <= hi; ++k) {
      const int32_t v = f[(int64_t)k * stride];
      best = v > best ? v : best;
    }
    out[b.off + q.p] = best;
  }
  if (mins) {
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) {
      const int32_t other = __shfl_xor(own, sft);
      own = other < own ? other : own;
    }
    if ((threadIdx.x & 63) == 0 && own != 0x7fffffff) atomicMin(&mins[blockIdx.y], own);
  }
}

// A block takes SP_CHUNK consecutive voxels of a box, 256 at a time.  EMIT false: the number of candidates among them; true: the
// candidates themselves at first[chunk] + their rank in the chunk, which is raster order.
template <bool EMIT>
__global__ void __launch_bounds__(SP_THREADS) split_cand_kernel(const int64_t* __restrict__ boxes, const int64_t* __restrict__ chunk0, int d,
                                                                const int32_t* __restrict__ d2, const int32_t* __restrict__ mx,
                                                                const int32_t* __restrict__ mins, int32_t* __restrict__ counts,
                                                                const int32_t* __restrict__ first, int32_t* __restrict__ cand, int64_t cap,
                                                                int32_t* __restrict__ box_counts) {
  __shared__ int wave_n[SP_WAVES];
  const SpBox b = sp_box(boxes + 8 * blockIdx.y);
  const int64_t chunks = (b.voxels() + SP_CHUNK - 1) / SP_CHUNK;
  if (blockIdx.x >= chunks) return;
  const int64_t chunk = chunk0[blockIdx.y] + blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t low = mins[blockIdx.y];
  if (EMIT && blockIdx.x == 0 && threadIdx.x == 0) box_counts[blockIdx.y] = first[chunk0[blockIdx.y] + chunks] - first[chunk];
  int64_t at = EMIT ? first[chunk] : 0;
  int total = 0;
  for (int i = 0; i < SP_CHUNK / SP_THREADS; ++i) {
    SpPos q;
    bool is = false;
    int32_t v = 0;
    if (sp_pos(b, (int64_t)blockIdx.x * SP_CHUNK + i * SP_THREADS + threadIdx.x, q)) {
      v = d2[b.off + q.p];
      is = v == mx[b.off + q.p] && v > low && (b.nx == 1 || (q.x >= d && q.x < b.nx - d)) && (b.ny == 1 || (q.y >= d && q.y < b.ny - d)) &&
           (b.nz == 1 || (q.z >= d && q.z < b.nz - d));
    }
    const uint64_t word = __ballot(is);
    if (lane == 0) wave_n[wave] = __popcll(word);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SP_WAVES; ++w) {
      before += w < wave ? wave_n[w] : 0;
      all += wave_n[w];
    }
    if (EMIT && is) {
      const int64_t slot = at + before + __popcll(word & ((1ull << lane) - 1));
      if (slot < cap) {
        cand[3 * slot] = (int32_t)blockIdx.y;
        cand[3 * slot + 1] = (int32_t)q.p;
        cand[3 * slot + 2] = v;
      }
    }
    at += all;
    total += all;
    __syncthreads();
  }
  if (!EMIT && threadIdx.x == 0) counts[chunk] = total;
}

// first[c] = the number of candidates in the chunks before c, for c in 0..n (n + 1 entries); one block walks the array
__global__ void __launch_bounds__(SP_THREADS) split_scan_kernel(const int32_t* __restrict__ counts, int64_t n, int32_t* __restrict__ first) {
  __shared__ int part[SP_THREADS];
  int carry = 0;
  for (int64_t c0 = 0; c0 < n; c0 += SP_THREADS) {
    const int64_t c = c0 + threadIdx.x;
    const int own = c < n ? counts[c] : 0;
    part[threadIdx.x] = own;
    __syncthreads();
    for (int s = 1; s < SP_THREADS; s <<= 1) {
      const int add = threadIdx.x >= s ? part[threadIdx.x - s] : 0;
      __syncthreads();
      part[threadIdx.x] += add;
      __syncthreads();
    }
    if (c < n) first[c] = carry + part[threadIdx.x] - own;
    carry += part[SP_THREADS - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) first[n] = carry;
}

// ---------------------------------------------------------------------------
// the flood
// ---------------------------------------------------------------------------
// A voxel's state: time = (L + 2^31) << 32 | g (SP_NEVER: not reached) and a label: -1 outside the mask, 0 not reached, else the
// marker's id, with SP_MARK on the marker voxels themselves.
__device__ __forceinline__ uint32_t sp_level(const int32_t* d2, int64_t i) { return d2 ? (uint32_t)(-d2[i]) ^ 0x80000000u : 0x80000000u; }

__global__ void __launch_bounds__(SP_THREADS) split_flood_init_kernel(const int64_t* __restrict__ boxes, const int32_t* __restrict__ mask_d2,
                                                                      uint64_t* __restrict__ time, int32_t* __restrict__ lab) {
  const SpBox b = sp_box(boxes + 8 * blockIdx.y);
  const int64_t p = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (p >= b.voxels()) return;
  time[b.off + p] = SP_NEVER;
  lab[b.off + p] = mask_d2[b.off + p] > 0 ? 0 : -1;
}

__global__ void __launch_bounds__(SP_THREADS) split_flood_seed_kernel(const int64_t* __restrict__ boxes, const int32_t* __restrict__ markers,
                                                                      int64_t n, const int32_t* __restrict__ energy_d2, uint64_t* __restrict__ time,
                                                                      int32_t* __restrict__ lab) {
  const int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (i >= n) return;
  const SpBox b = sp_box(boxes + 8 * markers[3 * i]);      // box, position and id were checked on the host
  const int64_t at = b.off + markers[3 * i + 1];
  if (lab[at] < 0) return;      // not a voxel of the label
  time[at] = (uint64_t)sp_level(energy_d2, at) << 32;
  lab[at] = markers[3 * i + 2] | SP_MARK;
}

__global__ void __launch_bounds__(SP_THREADS) split_flood_sweep_kernel(const int64_t* __restrict__ boxes, const int32_t* __restrict__ energy_d2,
                                                                       const uint64_t* __restrict__ time_in, const int32_t* __restrict__ lab_in,
                                                                       uint64_t* __restrict__ time_out, int32_t* __restrict__ lab_out,
                                                                       int32_t* __restrict__ changed) {
  const SpBox b = sp_box(boxes + 8 * blockIdx.y);
  SpPos q;
  if (!sp_pos(b, (int64_t)blockIdx.x * SP_THREADS + threadIdx.x, q)) return;
  const int64_t at = b.off + q.p;
  const uint64_t told = time_in[at];
  const int32_t lold = lab_in[at];
  uint64_t tnew = told;
  int32_t lnew = lold;
  if (lold >= 0 && !(lold & SP_MARK)) {
    uint64_t tb = SP_NEVER;
    int32_t lb = 0;
    const int64_t sy = b.nx, sz = (int64_t)b.nx * b.ny;
    const int64_t nb[6] = {q.z > 0 ? at - sz : -1,        q.y > 0 ? at - sy : -1,        q.x > 0 ? at - 1 : -1,
                           q.x < b.nx - 1 ? at + 1 : -1,  q.y < b.ny - 1 ? at + sy : -1, q.z < b.nz - 1 ? at + sz : -1};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      if (nb[k] < 0) continue;
      const uint64_t tp = time_in[nb[k]];
      if (tp == SP_NEVER) continue;      // outside the mask, or not reached
      const int32_t lp = lab_in[nb[k]] & SP_ID;
      if (tp < tb || (tp == tb && lp < lb)) {
        tb = tp;
        lb = lp;
      }
    }
    if (tb != SP_NEVER) {
      const uint32_t e = sp_level(energy_d2, at);
      tnew = e <= (uint32_t)(tb >> 32) ? tb + 1 : (uint64_t)e << 32;
      lnew = lb;
    }
  }
  time_out[at] = tnew;
  lab_out[at] = lnew;
  if (tnew != told || lnew != lold) *changed = 1;
}

__global__ void __launch_bounds__(SP_THREADS) split_flood_finish_kernel(const int64_t* __restrict__ boxes, const int32_t* __restrict__ lab,
                                                                        int32_t* __restrict__ out) {
  const SpBox b = sp_box(boxes + 8 * blockIdx.y);
  const int64_t p = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (p >= b.voxels()) return;
  const int32_t l = lab[b.off + p];
  out[b.off + p] = l < 0 ? 0 : l & SP_ID;
}

// ---------------------------------------------------------------------------
// labels[box][binary] = new[binary] + max_label (:544)
// ---------------------------------------------------------------------------
template <int S>
__global__ void __launch_bounds__(SP_THREADS) split_write_kernel(void* __restrict__ vol, int H, int W, const int64_t* __restrict__ boxes,
                                                                 const int32_t* __restrict__ marker, const int64_t* __restrict__ bases) {
  typedef typename SpElem<S>::type T;
  const SpBox b = sp_box(boxes + 8 * blockIdx.y);
  const int64_t base = bases[blockIdx.y];
  SpPos q;
  if (base < 0 || !sp_pos(b, (int64_t)blockIdx.x * SP_THREADS + threadIdx.x, q)) return;
  T* v = (T*)vol + ((int64_t)(b.z0 + q.z) * H + b.y0 + q.y) * W + b.x0 + q.x;
  if (*v == (T)b.label) *v = (T)(base + marker[b.off + q.p]);
}

// the boxes checked on the host and uploaded; *most = the voxels of the largest box, *flat = every box has nz == 1
int sp_boxes(const char* what, const int64_t* h_boxes, int n_boxes, int D, int H, int W, int64_t n_entries, int64_t* d_boxes, hipStream_t s,
             int64_t* most, bool* flat) {
  EMP_REQUIRE(h_boxes && d_boxes && n_boxes >= 1 && n_boxes <= SP_MAX_BOXES, "%s: 1..%d boxes (got %d)", what, SP_MAX_BOXES, n_boxes);
  EMP_REQUIRE(D >= 1 && H >= 1 && W >= 1 && n_entries >= 1 && n_entries < 0x7fffffffll, "%s: the boxes must hold fewer than 2^31 - 1 voxels", what);
  int64_t off = 0;
  *most = 0;
  *flat = true;
  for (int i = 0; i < n_boxes; ++i) {
    const int64_t* b = h_boxes + 8 * i;
    EMP_REQUIRE(b[3] >= 1 && b[4] >= 1 && b[5] >= 1 && b[0] >= 0 && b[1] >= 0 && b[2] >= 0 && b[0] + b[3] <= D && b[1] + b[4] <= H && b[2] + b[5] <= W,
                "%s: box %d is not inside the array", what, i);
    EMP_REQUIRE(b[3] * b[3] + b[4] * b[4] + b[5] * b[5] < (int64_t)SP_INF, "%s: box %d: nz^2 + ny^2 + nx^2 must be below 2^30", what, i);
    EMP_REQUIRE(b[6] == off, "%s: box %d: its entries must follow those of the box before", what, i);
    const int64_t v = b[3] * b[4] * b[5];
    off += v;
    EMP_REQUIRE(off <= n_entries, "%s: the boxes hold more than the %lld entries given", what, (long long)n_entries);
    *most = v > *most ? v : *most;
    *flat = *flat && b[3] == 1;
  }
  EMP_CHECK_HIP(hipMemcpyAsync(d_boxes, h_boxes, sizeof(int64_t) * 8 * n_boxes, hipMemcpyHostToDevice, s));
  return EMP_OK;
}

inline dim3 sp_grid(int64_t items, int per_block, int n_boxes) { return dim3((unsigned)((items + per_block - 1) / per_block), (unsigned)n_boxes); }

template <int S>
int sp_rows(const void* vol, int H, int W, const int64_t* d_boxes, int n_boxes, int64_t most_rows, int32_t* out, hipStream_t s) {
  hipLaunchKernelGGL((split_rows_kernel<S>), sp_grid(most_rows, SP_WAVES, n_boxes), dim3(SP_THREADS), 0, s, vol, H, W, d_boxes, out);
  EMP_LAUNCH_CHECK();
  return EMP_OK;
}

template <int S>
int sp_write(void* vol, int H, int W, const int64_t* d_boxes, int n_boxes, int64_t most, const int32_t* marker, const int64_t* bases, hipStream_t s) {
  hipLaunchKernelGGL((split_write_kernel<S>), sp_grid(most, SP_THREADS, n_boxes), dim3(SP_THREADS), 0, s, vol, H, W, d_boxes, marker, bases);
  EMP_LAUNCH_CHECK();
  return EMP_OK;
}

inline size_t sp_align(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace
}  // namespace emp

using namespace emp;

extern "C" {

size_t emp_split_edt_work_bytes(int64_t n_entries) { return n_entries < 1 ? 0 : 3 * sp_align(sizeof(int32_t) * (size_t)n_entries); }

int emp_split_edt(const void* d_vol, int elem_bytes, int D, int H, int W, const int64_t* h_boxes, int n_boxes, int64_t* d_boxes, int32_t* d_d2,
                  int64_t n_entries, void* d_work, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int64_t most;
  bool flat;
  if (int rc = sp_boxes("split_edt", h_boxes, n_boxes, D, H, W, n_entries, d_boxes, s, &most, &flat)) return rc;
  EMP_REQUIRE(d_vol && d_d2 && d_work, "split_edt: null array");
  const size_t part = sp_align(sizeof(int32_t) * (size_t)n_entries);
  int32_t* tmp = (int32_t*)d_work;
  int32_t* st = (int32_t*)((char*)d_work + part);
  int32_t* tt = (int32_t*)((char*)d_work + 2 * part);
  // images: rows -> tmp, y -> d2; volumes: rows -> d2, y -> tmp, z -> d2
  int32_t* rows = flat ? tmp : d_d2;
  int64_t most_rows = 0;
  for (int i = 0; i < n_boxes; ++i) most_rows = std::max(most_rows, h_boxes[8 * i + 3] * h_boxes[8 * i + 4]);
  const int A = elem_bytes < 0 ? -elem_bytes : elem_bytes;
  int rc;
  if (A == 1) rc = sp_rows<1>(d_vol, H, W, d_boxes, n_boxes, most_rows, rows, s);
  else if (A == 2) rc = sp_rows<2>(d_vol, H, W, d_boxes, n_boxes, most_rows, rows, s);
  else if (A == 4) rc = sp_rows<4>(d_vol, H, W, d_boxes, n_boxes, most_rows, rows, s);
  else if (A == 8) rc = sp_rows<8>(d_vol, H, W, d_boxes, n_boxes, most_rows, rows, s);
  else {
    set_error("split_edt: element size %d unsupported (1, 2, 4, 8; negative = signed)", elem_bytes);
    return EMP_ERR_INVALID;
  }
  if (rc) return rc;
  const dim3 grid = sp_grid(most, SP_THREADS, n_boxes), block(SP_THREADS);
  hipLaunchKernelGGL(split_env_kernel, grid, block, 0, s, (const int64_t*)d_boxes, 1, (const int32_t*)rows, flat ? d_d2 : tmp, st, tt);
  EMP_LAUNCH_CHECK();
  if (!flat) {
    hipLaunchKernelGGL(split_env_kernel, grid, block, 0, s, (const int64_t*)d_boxes, 0, (const int32_t*)tmp, d_d2, st, tt);
    EMP_LAUNCH_CHECK();
  }
  return EMP_OK;
}

static int64_t sp_chunks(const int64_t* h_boxes, int n_boxes) {
  int64_t n = 0;
  for (int i = 0; i < n_boxes; ++i) n += (h_boxes[8 * i + 3] * h_boxes[8 * i + 4] * h_boxes[8 * i + 5] + SP_CHUNK - 1) / SP_CHUNK;
  return n;
}

size_t emp_split_peaks_work_bytes(int64_t n_entries, int n_boxes) {
  if (n_entries < 1 || n_boxes < 1) return 0;
  const size_t chunks = (size_t)(n_entries / SP_CHUNK) + (size_t)n_boxes + 1;      // at most one ragged chunk per box
  return 2 * sp_align(sizeof(int32_t) * (size_t)n_entries) + sp_align(sizeof(int32_t) * (size_t)n_boxes) +
         sp_align(sizeof(int64_t) * ((size_t)n_boxes + 1)) + 2 * sp_align(sizeof(int32_t) * (chunks + 1));
}

int emp_split_peaks(const int64_t* h_boxes, int n_boxes, int64_t* d_boxes, int D, int H, int W, const int32_t* d_d2, int64_t n_entries,
                    int min_distance, int32_t* d_cand, int64_t cand_capacity, int32_t* d_box_counts, void* d_work, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int64_t most;
  bool flat;
  if (int rc = sp_boxes("split_peaks", h_boxes, n_boxes, D, H, W, n_entries, d_boxes, s, &most, &flat)) return rc;
  EMP_REQUIRE(d_d2 && d_cand && d_box_counts && d_work && cand_capacity >= 1, "split_peaks: null array");
  EMP_REQUIRE(min_distance >= 1 && min_distance <= 100, "split_peaks: min_distance 1..100 (got %d)", min_distance);
  const size_t part = sp_align(sizeof(int32_t) * (size_t)n_entries);
  const int64_t chunks = sp_chunks(h_boxes, n_boxes);
  char* w = (char*)d_work;
  int32_t* a = (int32_t*)w;
  int32_t* b = (int32_t*)(w + part);
  int32_t* mins = (int32_t*)(w + 2 * part);
  w += 2 * part + sp_align(sizeof(int32_t) * (size_t)n_boxes);
  int64_t* chunk0 = (int64_t*)w;
  w += sp_align(sizeof(int64_t) * ((size_t)n_boxes + 1));
  int32_t* counts = (int32_t*)w;
  int32_t* first = (int32_t*)(w + sp_align(sizeof(int32_t) * ((size_t)chunks + 1)));
  EMP_REQUIRE((size_t)((char*)(first + chunks + 1) - (char*)d_work) <= emp_split_peaks_work_bytes(n_entries, n_boxes), "split_peaks: work layout");
  {
    std::vector<int64_t> h0((size_t)n_boxes + 1);
    h0[0] = 0;
    for (int i = 0; i < n_boxes; ++i) h0[i + 1] = h0[i] + sp_chunks(h_boxes + 8 * i, 1);
    EMP_CHECK_HIP(hipMemcpyAsync(chunk0, h0.data(), sizeof(int64_t) * h0.size(), hipMemcpyHostToDevice, s));
    EMP_CHECK_HIP(hipStreamSynchronize(s));      // h0 goes out of scope
  }
  EMP_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)mins, 0x7fffffff, (size_t)n_boxes, s));
  const dim3 grid = sp_grid(most, SP_THREADS, n_boxes), block(SP_THREADS);
  hipLaunchKernelGGL(split_max_kernel, grid, block, 0, s, (const int64_t*)d_boxes, 2, min_distance, d_d2, a, mins);
  EMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(split_max_kernel, grid, block, 0, s, (const int64_t*)d_boxes, 1, min_distance, (const int32_t*)a, b, (int32_t*)nullptr);
  EMP_LAUNCH_CHECK();
  const int32_t* mx = b;
  if (!flat) {
    hipLaunchKernelGGL(split_max_kernel, grid, block, 0, s, (const int64_t*)d_boxes, 0, min_distance, (const int32_t*)b, a, (int32_t*)nullptr);
    EMP_LAUNCH_CHECK();
    mx = a;
  }
  const dim3 cgrid = sp_grid(most, SP_CHUNK, n_boxes);
  hipLaunchKernelGGL((split_cand_kernel<false>), cgrid, block, 0, s, (const int64_t*)d_boxes, (const int64_t*)chunk0, min_distance, d_d2, mx,
                     (const int32_t*)mins, counts, (const int32_t*)first, d_cand, cand_capacity, d_box_counts);
  EMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(split_scan_kernel, dim3(1), block, 0, s, (const int32_t*)counts, chunks, first);
  EMP_LAUNCH_CHECK();
  hipLaunchKernelGGL((split_cand_kernel<true>), cgrid, block, 0, s, (const int64_t*)d_boxes, (const int64_t*)chunk0, min_distance, d_d2, mx,
                     (const int32_t*)mins, counts, (const int32_t*)first, d_cand, cand_capacity, d_box_counts);
  EMP_LAUNCH_CHECK();
  return EMP_OK;
}

size_t emp_split_flood_work_bytes(int64_t n_entries, int64_t n_markers) {
  if (n_entries < 1 || n_markers < 0) return 0;
  return 2 * sp_align(sizeof(uint64_t) * (size_t)n_entries) + 2 * sp_align(sizeof(int32_t) * (size_t)n_entries) +
         sp_align(sizeof(int32_t) * 3 * (size_t)(n_markers + 1)) + sp_align(sizeof(int32_t) * SP_BATCH);
}

int emp_split_flood(const int64_t* h_boxes, int n_boxes, int64_t* d_boxes, int D, int H, int W, const int32_t* d_d2, int64_t n_entries, int plateau,
                    const int32_t* h_markers, int64_t n_markers, int32_t* d_out, void* d_work, void* stream, int64_t* h_sweeps) {
  hipStream_t s = (hipStream_t)stream;
  int64_t most;
  bool flat;
  if (int rc = sp_boxes("split_flood", h_boxes, n_boxes, D, H, W, n_entries, d_boxes, s, &most, &flat)) return rc;
  EMP_REQUIRE(d_d2 && d_out && d_work && h_sweeps && n_markers >= 0 && (h_markers || n_markers == 0), "split_flood: null array");
  for (int64_t i = 0; i < n_markers; ++i) {
    const int32_t* m = h_markers + 3 * i;
    EMP_REQUIRE(m[0] >= 0 && m[0] < n_boxes && m[1] >= 0 && m[1] < h_boxes[8 * m[0] + 3] * h_boxes[8 * m[0] + 4] * h_boxes[8 * m[0] + 5] &&
                    m[2] >= 1 && m[2] <= SP_ID,
                "split_flood: marker %lld is not in its box, or its id is not in 1..2^30 - 1", (long long)i);
  }
  const size_t tpart = sp_align(sizeof(uint64_t) * (size_t)n_entries), lpart = sp_align(sizeof(int32_t) * (size_t)n_entries);
  char* w = (char*)d_work;
  uint64_t* time[2] = {(uint64_t*)w, (uint64_t*)(w + tpart)};
  int32_t* lab[2] = {(int32_t*)(w + 2 * tpart), (int32_t*)(w + 2 * tpart + lpart)};
  int32_t* markers = (int32_t*)(w + 2 * tpart + 2 * lpart);
  int32_t* flags = (int32_t*)((char*)markers + sp_align(sizeof(int32_t) * 3 * (size_t)(n_markers + 1)));
  const int32_t* energy = plateau ? nullptr : d_d2;
  const dim3 grid = sp_grid(most, SP_THREADS, n_boxes), block(SP_THREADS);
  hipLaunchKernelGGL(split_flood_init_kernel, grid, block, 0, s, (const int64_t*)d_boxes, d_d2, time[0], lab[0]);
  EMP_LAUNCH_CHECK();
  if (n_markers) {
    EMP_CHECK_HIP(hipMemcpyAsync(markers, h_markers, sizeof(int32_t) * 3 * (size_t)n_markers, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(split_flood_seed_kernel, dim3((unsigned)((n_markers + SP_THREADS - 1) / SP_THREADS)), block, 0, s, (const int64_t*)d_boxes,
                       (const int32_t*)markers, n_markers, energy, time[0], lab[0]);
    EMP_LAUNCH_CHECK();
  }
  // a claim chain is shorter than the boxes' voxels: more sweeps than that cannot change anything
  int64_t sweeps = 0;
  int cur = 0;
  bool still = true;
  while (still) {
    EMP_REQUIRE(sweeps <= n_entries + SP_BATCH, "split_flood: no fixed point after %lld sweeps", (long long)sweeps);
    EMP_CHECK_HIP(hipMemsetAsync(flags, 0, sizeof(int32_t) * SP_BATCH, s));
    for (int k = 0; k < SP_BATCH; ++k) {
      hipLaunchKernelGGL(split_flood_sweep_kernel, grid, block, 0, s, (const int64_t*)d_boxes, energy, (const uint64_t*)time[cur],
                         (const int32_t*)lab[cur], time[cur ^ 1], lab[cur ^ 1], flags + k);
      EMP_LAUNCH_CHECK();
      cur ^= 1;
    }
    int32_t h_flags[SP_BATCH];
    EMP_CHECK_HIP(hipMemcpyAsync(h_flags, flags, sizeof(h_flags), hipMemcpyDeviceToHost, s));
    EMP_CHECK_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < SP_BATCH && still; ++k) {
      ++sweeps;
      still = h_flags[k] != 0;
    }
  }
  // after a sweep that changed nothing both buffers hold the fixed point
  hipLaunchKernelGGL(split_flood_finish_kernel, grid, block, 0, s, (const int64_t*)d_boxes, (const int32_t*)lab[cur], d_out);
  EMP_LAUNCH_CHECK();
  *h_sweeps = sweeps;
  return EMP_OK;
}

int emp_split_write(void* d_vol, int elem_bytes, int D, int H, int W, const int64_t* h_boxes, int n_boxes, int64_t* d_boxes,
                    const int32_t* d_markers, int64_t n_entries, const int64_t* d_bases, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int64_t most;
  bool flat;
  if (int rc = sp_boxes("split_write", h_boxes, n_boxes, D, H, W, n_entries, d_boxes, s, &most, &flat)) return rc;
  EMP_REQUIRE(d_vol && d_markers && d_bases, "split_write: null array");
  const int A = elem_bytes < 0 ? -elem_bytes : elem_bytes;
  if (A == 1) return sp_write<1>(d_vol, H, W, d_boxes, n_boxes, most, d_markers, d_bases, s);
  if (A == 2) return sp_write<2>(d_vol, H, W, d_boxes, n_boxes, most, d_markers, d_bases, s);
  if (A == 4) return sp_write<4>(d_vol, H, W, d_boxes, n_boxes, most, d_markers, d_bases, s);
  if (A == 8) return sp_write<8>(d_vol, H, W, d_boxes, n_boxes, most, d_markers, d_bases, s);
  set_error("split_write: element size %d unsupported (1, 2, 4, 8; negative = signed)", elem_bytes);
  return EMP_ERR_INVALID;
}

}  // extern "C"
