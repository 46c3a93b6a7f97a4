// Contact Labels on the device: per unordered pair {a, b} of different label values that occur next to each other, how many
// voxel pairs join them along each of the 13 half-directions of the 26-neighbourhood -- the integers behind the area of the
// surface two objects share and behind a region adjacency graph.  There is no counterpart in the reference plugin; the nearest
// thing is skimage's region adjacency graph (skimage.graph.RAG, rag_boundary).  skimage is not available where this library is
// built: nothing is pinned against it, the tests state the definition in numpy.  Everything is an integer, so the result is exact
// and does not depend on how the volume is cut into slabs.
//
//   N[k]     the half-directions d_k are the (dz, dy, dx) in {-1, 0, 1}^3 \ {0} whose first non-zero component is +1, in
//            ascending lexicographic order (CT_DIR; shape.hip's): #{p : p and p + d_k both in the array, {L(p), L(p + d_k)} =
//            {a, b}}.  A pair with an end outside the array is never counted.
//   count    sum_k N[k]: a pair exists exactly if its count is positive.
//   key      min(a, b) << 32 | max(a, b), labels in [0, 2^32); a != b, so a key never equals CELL_EMPTY.  A pair with a 0 in
//            it (the background) is entered, under (0, b), only when `background` is set.
// Summed over the partners b of a label a, 0 included, N[k](a, b) is shape.hip's intercepts[k] of a without border faces.
//
// One kernel per slab, in the shape of label_shape_kernel (shape.hip), restated here: 256 threads; 16-byte loads, one vector per
// lane; a tile's first voxel carried along the workgroup's stretch of tiles, at most 2048 workgroups; a bounded-probe LDS table
// per workgroup, flushed once with one global update per occupied slot; no loop waits for another lane, wave or workgroup.  A
// voxel p is the LATER end of its 13 pairs (p - d_k, p), so a lane reads its own E voxels, the row above and the three rows
// around them in the slice below, each as a window of E + 2 elements (the two ends come from the neighbouring lanes).  The two
// rules everything rests on:
//   * RAVELED WINDOWS.  A window is a stretch of the raveled slab.  x - 1 at x = 0 and x + 1 at x = W - 1 are the ends of the
//     neighbouring rows there, but they lie outside the array; the same holds for y - 1 at y = 0 and y + 1 at y = H - 1 across
//     slices.  A neighbour counts only where its coordinates lie in the array.
//   * SEAM PAIRS.  The pairs across a slab's lower border come from the halo slice (for z0 == 0 there is no slice below).  They
//     are counted by the upper slab only -- no slab looks at the slice above its last one -- so no pair is counted twice or
//     dropped, whatever the slab size.
// A lane whose voxels and windows are all one value does nothing at all: there is no count to carry.  A lane merges consecutive
// credits to one key in registers (CtAcc) before it touches LDS; along the face between two objects that is every credit of the
// lane.  When the LDS neighbourhood of a key is full the credit goes straight to the global table; when the global one is full
// the overflow flag is raised and the credit dropped (the host undoes the slab and grows the table).  Every column is an add
// modulo 2^64, so the same slab with negated weights takes out exactly what a failed call added.
// A slot is 120 bytes (key, count, 13 x u64): 256 LDS slots are 30 KiB per workgroup.  The windows are kept in 32 bits per voxel
// unless the labels have 64.  The loop over a lane's voxels has to be unrolled in full or the windows are indexed at run time
// and live in scratch memory: build.py raises the size up to which `#pragma unroll` is obeyed for this file, as for shape.hip.
// ct_flush is a call (13 places per voxel could need it), made only by lanes that change their key.  Registers: 155 / 114 / 101 /
// 134 VGPRs for 1- / 2- / 4- / 8-byte labels (three, four, four, three waves per SIMD) and 224 bytes of scratch per lane, the
// call's frame.
// The table around the count kernel is label_table.h's; ContactCells tells it what a cell of this family is.
#include "common.h"
#include "label_table.h"

namespace emp {
namespace {

constexpr int CT_THREADS = 256;
constexpr int CT_LDS_SLOTS = 256;
constexpr int CT_LDS_PROBES = 8;
constexpr int CT_GLOBAL_PROBES = 128;
constexpr int64_t CT_MAX_GRID = 2048;      // two rounds of the 1024 workgroups the chip holds
constexpr uint64_t CT_EMPTY = CELL_EMPTY;  // a key has a != b: never all ones
constexpr int CT_DIRS = 13;

typedef unsigned long long ull_t;

// (dz, dy, dx) of the half-directions: first non-zero component +1, lexicographic
struct CtDirs {
  int d[CT_DIRS][3];
  constexpr CtDirs() : d() {
    int k = 0;
    for (int z = -1; z <= 1; ++z)
      for (int y = -1; y <= 1; ++y)
        for (int x = -1; x <= 1; ++x) {
          const int first = z ? z : (y ? y : x);
          if (first > 0) {
            d[k][0] = z;
            d[k][1] = y;
            d[k][2] = x;
            ++k;
          }
        }
  }
};
constexpr CtDirs CT_DIR;
static_assert(CT_DIR.d[0][2] == 1 && CT_DIR.d[2][1] == 1 && CT_DIR.d[8][0] == 1 && CT_DIR.d[8][1] == 0 && CT_DIR.d[8][2] == 0 && CT_DIR.d[12][2] == 1,
              "the axis directions are columns 8, 2, 0");

struct CtTable {
  uint64_t* hdr;
  uint64_t* keys;
  uint64_t* counts;
  uint64_t* pairs;
  uint64_t mask;
};

// what an LDS slot or a cell adds to a cell
struct CtRec {
  uint64_t cnt;
  uint64_t n[CT_DIRS];
};

// the cell of `key`, claimed if need be; -1 and the overflow flag when the probes run out
__device__ __forceinline__ int64_t ct_global_find(const CtTable& t, uint64_t key) {
  uint64_t s = ov_hash(key) & t.mask;
#pragma unroll 1
  for (int p = 0; p < CT_GLOBAL_PROBES; ++p) {
    uint64_t cur = __hip_atomic_load(&t.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == CT_EMPTY) {
      cur = atomicCAS((ull_t*)&t.keys[s], (ull_t)CT_EMPTY, (ull_t)key);
      if (cur == CT_EMPTY) cur = key;
    }
    if (cur == key) return (int64_t)s;
    s = (s + 1) & t.mask;
  }
  atomicOr((unsigned int*)&t.hdr[1], 1u);      // dropped: the host undoes the slab and grows the table
  return -1;
}

// negate: the undo pass -- every column with the opposite sign
__device__ __forceinline__ void ct_global_add(const CtTable& t, uint64_t key, const CtRec& r, int negate) {
  const int64_t s = ct_global_find(t, key);
  if (s < 0) return;
  if (r.cnt) atomicAdd((ull_t*)&t.counts[s], (ull_t)(negate ? 0ull - r.cnt : r.cnt));
#pragma unroll
  for (int k = 0; k < CT_DIRS; ++k)
    if (r.n[k]) atomicAdd((ull_t*)&t.pairs[s * CT_DIRS + k], (ull_t)(negate ? 0ull - r.n[k] : r.n[k]));
}

struct CtCtx {
  uint64_t* lkeys;
  uint64_t* lcnt;
  uint64_t* lpairs;
  CtTable t;
  uint32_t H, W;
  float invH, invW;
  int negate;
};

__device__ __forceinline__ int ct_lds_find(const CtCtx& c, uint64_t key) {
  uint32_t s = (uint32_t)ov_hash(key) & (CT_LDS_SLOTS - 1);
#pragma unroll 1
  for (int p = 0; p < CT_LDS_PROBES; ++p) {
    uint64_t cur = __hip_atomic_load(&c.lkeys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (cur == CT_EMPTY) {
      cur = atomicCAS((ull_t*)&c.lkeys[s], (ull_t)CT_EMPTY, (ull_t)key);
      if (cur == CT_EMPTY) cur = key;
    }
    if (cur == key) return (int)s;
    s = (s + 1) & (CT_LDS_SLOTS - 1);
  }
  return -1;
}

// what a lane has gathered for one key; key CT_EMPTY: nothing yet
struct CtAcc {
  uint64_t key;
  uint32_t n[CT_DIRS];
};

__device__ __forceinline__ void ct_clear(CtAcc& a, uint64_t key) {
  a.key = key;
#pragma unroll
  for (int k = 0; k < CT_DIRS; ++k) a.n[k] = 0;
}

// the lane's credits for a.key into the workgroup's table, or into the global one when the LDS probes run out.  A call, not
// inlined: the loop over a lane's voxels is unrolled and every direction of every voxel may have to flush
__device__ __noinline__ void ct_flush(const CtCtx& c, const CtAcc a) {
  if (a.key == CT_EMPTY) return;
  uint32_t total = 0;
#pragma unroll
  for (int k = 0; k < CT_DIRS; ++k) total += a.n[k];
  const int s = ct_lds_find(c, a.key);
  if (s < 0) {
    CtRec r;
    r.cnt = total;
#pragma unroll
    for (int k = 0; k < CT_DIRS; ++k) r.n[k] = a.n[k];
    ct_global_add(c.t, a.key, r, c.negate);
    return;
  }
  atomicAdd((ull_t*)&c.lcnt[s], (ull_t)total);
#pragma unroll
  for (int k = 0; k < CT_DIRS; ++k)
    if (a.n[k]) atomicAdd((ull_t*)&c.lpairs[s * CT_DIRS + k], (ull_t)a.n[k]);
}

// A lane keeps its windows in 32 bits per voxel unless the labels have 64
template <int S> struct CtVal { typedef uint32_t type; };
template <> struct CtVal<8> { typedef uint64_t type; };

__device__ __forceinline__ uint32_t ct_shfl_up(uint32_t v) { return (uint32_t)__shfl_up((unsigned int)v, 1); }
__device__ __forceinline__ uint64_t ct_shfl_up(uint64_t v) { return (uint64_t)__shfl_up((ull_t)v, 1); }
__device__ __forceinline__ uint32_t ct_shfl_down(uint32_t v) { return (uint32_t)__shfl_down((unsigned int)v, 1); }
__device__ __forceinline__ uint64_t ct_shfl_down(uint64_t v) { return (uint64_t)__shfl_down((ull_t)v, 1); }

// values outside the domain of half a key, [0, 2^32): a high word (a negative 8-byte value has one), a negative signed value
template <int S>
__device__ __forceinline__ bool ct_out_of_range(uint64_t v, int is_signed) {
  if (S == 8) return (v >> 32) != 0;
  return is_signed && ((v >> (8 * S - 1)) & 1);
}

// where the windows of a lane come from: the slab (n voxels) and the slice below its first one (HW voxels, or null)
template <int S>
struct CtSrc {
  typedef typename OvElem<S>::type T;
  typedef typename CtVal<S>::type WT;
  const T* a;
  const T* halo;
  int64_t n, HW;
  // the voxel at raveled index i of the slab; [-HW, 0) is the halo slice; anything else, and a missing halo, reads as 0
  __device__ __forceinline__ WT at(int64_t i) const {
    if (i >= 0) return i < n ? (WT)a[i] : (WT)0;
    return (halo && i >= -HW) ? (WT)halo[i + HW] : (WT)0;
  }
};

// w[0 .. E + 1] = the voxels s - 1 .. s + E of the raveled slab: the E in the middle by one vector load where they lie in one
// array and the address allows it, the two ends from the neighbouring lanes (whose windows start E voxels before and after
// this one; the bounds are those of the source alone, so every lane of the wave holds what its neighbour asks for)
template <int S, int E>
__device__ __forceinline__ void ct_window(const CtSrc<S>& src, int64_t s, int lane, typename CtVal<S>::type* w) {
  typedef typename OvElem<S>::type T;
  typedef typename OvVec<S * E>::type V;
  typedef typename CtVal<S>::type WT;
  const T* p = nullptr;
  if (s >= 0 && s + E <= src.n)
    p = src.a + s;
  else if (src.halo && s >= -src.HW && s + E <= 0)
    p = src.halo + (s + src.HW);
  if (p && (uintptr_t)p % (S * E) == 0) {
    const V vec = *(const V*)p;
    T e[E];
    __builtin_memcpy(e, &vec, sizeof(vec));
#pragma unroll
    for (int j = 0; j < E; ++j) w[1 + j] = (WT)e[j];
  } else {
#pragma unroll
    for (int j = 0; j < E; ++j) w[1 + j] = src.at(s + j);
  }
  w[0] = ct_shfl_up(w[E]);
  w[E + 1] = ct_shfl_down(w[1]);
  if (lane == 0) w[0] = src.at(s - 1);
  if (lane == 63) w[E + 1] = src.at(s + E);
}

// a: the slab (n voxels); halo: the slice below its first one (H * W voxels) or null; zoff: the slab's first slice
template <int S>
__global__ void __launch_bounds__(CT_THREADS) label_contacts_kernel(const void* __restrict__ a, const void* __restrict__ halo, int64_t n,
                                                                    int is_signed, int64_t tiles_per_wg, CtTable t, uint32_t H, uint32_t W,
                                                                    uint32_t zoff, float invH, float invW, int background, int negate) {
  typedef typename OvElem<S>::type T;
  typedef typename CtVal<S>::type WT;
  constexpr int E = 16 / S;
  constexpr uint32_t TILE = CT_THREADS * E;
  __shared__ uint64_t lkeys[CT_LDS_SLOTS];
  __shared__ uint64_t lcnt[CT_LDS_SLOTS];
  __shared__ uint64_t lpairs[CT_LDS_SLOTS * CT_DIRS];
  for (int i = threadIdx.x; i < CT_LDS_SLOTS; i += CT_THREADS) {
    lkeys[i] = CT_EMPTY;
    lcnt[i] = 0;
#pragma unroll
    for (int k = 0; k < CT_DIRS; ++k) lpairs[i * CT_DIRS + k] = 0;
  }
  __syncthreads();
  CtCtx c;
  c.lkeys = lkeys;
  c.lcnt = lcnt;
  c.lpairs = lpairs;
  c.t = t;
  c.H = H;
  c.W = W;
  c.invH = invH;
  c.invW = invW;
  c.negate = negate;
  const int lane = threadIdx.x & 63;
  CtSrc<S> src;
  src.a = (const T*)a;
  src.halo = (const T*)halo;
  src.n = n;
  src.HW = (int64_t)H * W;
  const int64_t HW = src.HW;
  const int64_t ntiles = (n + TILE - 1) / TILE;
  const int64_t tile0 = (int64_t)blockIdx.x * tiles_per_wg;
  const int64_t tile1 = tile0 + tiles_per_wg < ntiles ? tile0 + tiles_per_wg : ntiles;
  // (bz, by, bx): the first voxel of the current tile, carried from tile to tile
  const int64_t row0 = tile0 * TILE / W;
  uint32_t bx = (uint32_t)(tile0 * TILE - row0 * W), bz = (uint32_t)(row0 / H), by = (uint32_t)(row0 - (int64_t)bz * H);
  bool bad = false;
  for (int64_t tile = tile0; tile < tile1; ++tile) {
    const uint32_t o0 = threadIdx.x * E;
    const int64_t i0 = tile * TILE + o0;
    const int64_t left = n - i0;
    const int nv = left >= E ? E : (left > 0 ? (int)left : 0);
    // win[dz ? 3 + dy : dy][1 + j - dx]: the neighbour (z - dz, y - dy, x - dx) of the lane's voxel j, where it lies in the array;
    // rows: 0 the voxels' own (only dx = 1 is asked of it), 1 the row above, 2 .. 4 the rows y + 1, y, y - 1 of the slice below
    WT win[5][E + 2];
    ct_window<S, E>(src, i0, lane, win[0]);
    ct_window<S, E>(src, i0 - (int64_t)W, lane, win[1]);
    ct_window<S, E>(src, i0 - HW + (int64_t)W, lane, win[2]);
    ct_window<S, E>(src, i0 - HW, lane, win[3]);
    ct_window<S, E>(src, i0 - HW - (int64_t)W, lane, win[4]);
    const WT* v = &win[0][1];
    bool flat = win[0][0] == v[0];      // the voxels the lane holds (those beyond the slab read as 0) and all their windows are one value
#pragma unroll
    for (int j = 0; j < E; ++j) {
      bad = bad || (j < nv && ct_out_of_range<S>(v[j], is_signed));
      flat &= v[j] == v[0];
    }
#pragma unroll
    for (int j = 0; j < E + 2; ++j) flat &= win[1][j] == v[0] && win[2][j] == v[0] && win[3][j] == v[0] && win[4][j] == v[0];
    if (nv > 0 && !flat) {
      uint32_t x, y, z;
      ov_coord(c, bx, by, bz, o0, x, y, z);
      CtAcc acc;
      ct_clear(acc, CT_EMPTY);
#pragma unroll
      for (int j = 0; j < E; ++j) {
        if (j < nv) {
          const WT own = v[j];
          // which neighbours exist: low[a] the one at index - 1, high[a] the one at index + 1 of axis a (z, y, x); the slab has
          // no slice above a voxel that it looks at, and the one below slice 0 of the volume does not exist
          const bool low[3] = {zoff + z > 0, y > 0, x > 0};
          const bool high[2] = {y + 1 < H, x + 1 < W};
#pragma unroll
          for (int k = 0; k < CT_DIRS; ++k) {
            const int dz = CT_DIR.d[k][0], dy = CT_DIR.d[k][1], dx = CT_DIR.d[k][2];
            // p - d: dz, dy, dx = 1 step to the lower index, -1 to the higher one
            const bool inside = (dz == 0 || low[0]) && (dy == 0 || (dy > 0 ? low[1] : high[0])) && (dx == 0 || (dx > 0 ? low[2] : high[1]));
            const WT nb = win[dz ? 3 + dy : dy][1 + j - dx];
            bool pair = inside && nb != own && (background || (nb != 0 && own != 0));
            if (S == 8) pair = pair && ((uint64_t)(own | nb) >> 32) == 0;      // the call fails on such a value: keep the key well formed
            if (pair) {
              const uint64_t lo = own < nb ? own : nb, hi = own < nb ? nb : own;
              const uint64_t key = (lo << 32) | hi;
              if (acc.key != key) {
                ct_flush(c, acc);
                ct_clear(acc, key);
              }
              ++acc.n[k];
            }
          }
          if (++x == W) {
            x = 0;
            if (++y == H) {
              y = 0;
              ++z;
            }
          }
        }
      }
      ct_flush(c, acc);
    }
    ov_coord(c, bx, by, bz, TILE, bx, by, bz);
  }
  if (bad) atomicOr((unsigned int*)&t.hdr[1] + 1, 1u);
  __syncthreads();
  for (int i = threadIdx.x; i < CT_LDS_SLOTS; i += CT_THREADS) {
    const uint64_t k = lkeys[i];
    if (k == CT_EMPTY) continue;
    CtRec r;
    r.cnt = lcnt[i];
#pragma unroll
    for (int f = 0; f < CT_DIRS; ++f) r.n[f] = lpairs[i * CT_DIRS + f];
    if (r.cnt) ct_global_add(t, k, r, negate);
  }
}

// a cell is a key, a count and 13 x u64
struct ContactCells {
  typedef CtTable Table;
  struct Out {
    uint64_t* keys;
    uint64_t* counts;
    uint64_t* pairs;
  };
  static constexpr size_t SLOT_BYTES = 16 + 8 * CT_DIRS;
  static constexpr int HEADER_CELLS = 0;
  static void layout(CtTable& t, int64_t capacity) { t.pairs = t.counts + capacity; }
  static __device__ void clear(const CtTable& t, int64_t i) {
    for (int k = 0; k < CT_DIRS; ++k) t.pairs[i * CT_DIRS + k] = 0;
  }
  static __device__ void move(const CtTable& from, int64_t i, uint64_t key, uint64_t w, const CtTable& to) {
    CtRec r;
    r.cnt = w;
    for (int k = 0; k < CT_DIRS; ++k) r.n[k] = from.pairs[i * CT_DIRS + k];
    ct_global_add(to, key, r, 0);
  }
  static __device__ void write(const CtTable& t, int64_t i, const Out& out, int64_t pos) {
    for (int k = 0; k < CT_DIRS; ++k) out.pairs[pos * CT_DIRS + k] = t.pairs[i * CT_DIRS + k];
  }
};
static_assert(ContactCells::SLOT_BYTES == 120, "key, count, 13 x u64");

struct CtSlab {
  const void* a;
  const void* halo;
  int64_t n, z0;
  int H, W, background;
};

template <int S>
int ct_launch(const CtSlab& g, int is_signed, const CtTable& t, int negate, hipStream_t s) {
  constexpr int64_t TILE = (int64_t)CT_THREADS * (16 / S);
  const int64_t ntiles = (g.n + TILE - 1) / TILE;
  const int64_t per = (ntiles + CT_MAX_GRID - 1) / CT_MAX_GRID;
  const int grid = (int)((ntiles + per - 1) / per);
  hipLaunchKernelGGL((label_contacts_kernel<S>), dim3(grid), dim3(CT_THREADS), 0, s, g.a, g.halo, g.n, is_signed, per, t, (uint32_t)g.H,
                     (uint32_t)g.W, (uint32_t)g.z0, 1.0f / (float)g.H, 1.0f / (float)g.W, g.background, negate);
  EMP_LAUNCH_CHECK();
  return EMP_OK;
}

int ct_dispatch(const CtSlab& g, int in_bytes, const CtTable& t, int negate, hipStream_t s) {
  const int sg = in_bytes < 0, A = sg ? -in_bytes : in_bytes;
  if (A == 1) return ct_launch<1>(g, sg, t, negate, s);
  if (A == 2) return ct_launch<2>(g, sg, t, negate, s);
  if (A == 4) return ct_launch<4>(g, sg, t, negate, s);
  if (A == 8) return ct_launch<8>(g, sg, t, negate, s);
  set_error("label_contacts: element size %d unsupported (1, 2, 4, 8; negative = signed)", in_bytes);
  return EMP_ERR_INVALID;
}

}  // namespace
}  // namespace emp

using namespace emp;

extern "C" {

size_t emp_label_contacts_work_bytes(int64_t capacity) {
  return cells_capacity_ok(capacity) ? CELL_HEADER + (size_t)capacity * ContactCells::SLOT_BYTES : 0;
}

int emp_label_contacts_reset(void* d_table, int64_t capacity, void* stream) {
  EMP_REQUIRE(d_table && cells_capacity_ok(capacity), "label_contacts_reset: the capacity must be a power of two in [64, 2^32]");
  return cells_reset<ContactCells>(d_table, capacity, (hipStream_t)stream);
}

// Synchronises the stream (it reads the table's flags).  *h_overflow = 1: the table was too small for this slab; what the call
// had added has been taken out again.
int emp_label_contacts_accumulate(const void* d_labels, int in_bytes, int64_t z0, int depth, int H, int W, int64_t total_depth,
                                  const void* d_halo, int background, void* d_table, int64_t capacity, void* stream, int* h_overflow) {
  EMP_REQUIRE(d_table && cells_capacity_ok(capacity) && h_overflow && depth >= 0 && H > 0 && W > 0 && (depth == 0 || d_labels),
              "label_contacts_accumulate: bad arguments");
  EMP_REQUIRE(z0 >= 0 && total_depth >= z0 + depth, "label_contacts_accumulate: the slab [%lld, %lld) does not lie in a volume of depth %lld",
              (long long)z0, (long long)(z0 + depth), (long long)total_depth);
  EMP_REQUIRE(total_depth < (1ll << 31) && H < (1 << 30) && W < (1 << 30), "label_contacts_accumulate: shape (%lld, %d, %d) beyond 2^31, 2^30, 2^30",
              (long long)total_depth, H, W);
  EMP_REQUIRE(z0 == 0 || depth == 0 || d_halo, "label_contacts_accumulate: a slab that starts at slice %lld needs the slice below it (d_halo)",
              (long long)z0);
  hipStream_t s = (hipStream_t)stream;
  *h_overflow = 0;
  CtSlab g;
  g.a = d_labels;
  g.halo = z0 == 0 ? nullptr : d_halo;
  g.n = (int64_t)depth * H * W;
  g.z0 = z0;
  g.H = H;
  g.W = W;
  g.background = background != 0;
  if (g.n == 0) return EMP_OK;
  const CtTable t = cells_table<ContactCells>(d_table, capacity);
  return cells_accumulate(t.hdr, s, "label_contacts_accumulate", "the key's domain (negative, or beyond 2^32)",
                          [&](int negate) { return ct_dispatch(g, in_bytes, t, negate, s); }, h_overflow);
}

// Moves the cells of a table into an empty (reset) larger one.  Synchronises; *h_overflow = 1: d_to is too small as well.
int emp_label_contacts_grow(const void* d_from, int64_t from_capacity, void* d_to, int64_t to_capacity, void* stream, int* h_overflow) {
  EMP_REQUIRE(d_from && d_to && cells_capacity_ok(from_capacity) && cells_capacity_ok(to_capacity) && to_capacity > from_capacity && h_overflow,
              "label_contacts_grow: bad arguments");
  return cells_grow<ContactCells>(d_from, from_capacity, d_to, to_capacity, (hipStream_t)stream, h_overflow);
}

// Synchronises.  *h_num = number of keys; the first min(*h_num, max_out) of them are written.
int emp_label_contacts_finalize(void* d_table, int64_t capacity, uint64_t* d_keys, uint64_t* d_counts, uint64_t* d_pairs, int64_t max_out,
                                int64_t* h_num, void* stream) {
  EMP_REQUIRE(d_table && cells_capacity_ok(capacity) && h_num && max_out >= 0 && (max_out == 0 || (d_keys && d_counts && d_pairs)),
              "label_contacts_finalize: bad arguments");
  return cells_finalize<ContactCells>(d_table, capacity, {d_keys, d_counts, d_pairs}, max_out, h_num, (hipStream_t)stream);
}

}  // extern "C"
