// Shape Labels on the device: per label that occurs (0, the background, excepted) the voxel count, the intercept counts along the
// 13 half-directions of the 26-neighbourhood and the Euler number under full and under face connectivity -- the integers behind a
// Cauchy-Crofton surface (skimage's perimeter_crofton, and the same estimator one dimension up) and euler_number.  skimage is not
// available where this library is built: both are restated from their documented behaviour, not pinned against them.  Everything
// is an integer, so the result is exact and does not depend on how the volume is cut into slabs.
//
//   intercepts[k]  the half-directions d_k are the (dz, dy, dx) in {-1, 0, 1}^3 \ {0} whose first non-zero component is +1, in
//                  ascending lexicographic order (SH_DIR); with M the voxels of a label, #{p in M : p + d_k not in M} +
//                  #{p in M : p - d_k not in M}.  border 1: a neighbour outside the array is not in M; 0: a pair with one end
//                  outside is not counted.  The axis directions (k = 8, 2, 0 for z, y, x) are measure.hip's faces.
//   euler[0]       V - E + F - C of the union of the closed voxel cubes of M (full connectivity);
//   euler[1]       voxels - face pairs + 2 x 2 quads - 2 x 2 x 2 octets inside M (face connectivity).
// Both Euler numbers are sums over the vertices c of the voxel grid, [0, D] x [0, H] x [0, W], of a small signed integer that
// depends only on which of the 8 voxels around c (c - t, t in {0, 1}^3; outside the array: background) belong to M: the vertex
// owns itself, the 3 edges, 3 faces and the voxel that lead from it towards lower indices, and the voxel c - 1 with the pairs,
// quads and the octet it is the lowest member of.  ShEulerTable is made from exactly these two definitions at compile time.
// Per slice (a stack of images) everything is the 2-D statement: the first four directions, 4 pixels around a vertex.
//
// One kernel per slab.  It follows label_measure_kernel (measure.hip): 16-byte loads, one vector per lane; a tile's first voxel
// carried along the workgroup's stretch of tiles; a bounded-probe LDS table per workgroup, flushed with one global update per
// occupied slot; no loop waits for another lane.  A voxel p is the LATER end of its 13 pairs (p, p - d_k) and the highest voxel
// of the vertex c = p, so a lane reads its own E voxels, the row above and the three rows around them in the slice below -- the
// latter from the halo slice for the slab's first slice -- each as a window of E + 2 elements (the two ends come from the
// neighbouring lanes).  What differs from measure:
//   * a window is a stretch of the RAVELED slab.  x - 1 at x = 0 and x + 1 at x = W - 1 are the ends of the neighbouring rows
//     there, but outside the array: a neighbour is taken from its window only where its coordinates lie in the array.
//   * the vertices on the high faces of the array (z = D, y = H, x = W) have no voxel p = c: the voxels at the last index of an
//     axis process them as well (c = p + e), with the outside as background; for z only in the slab that holds the last slice.
//   * a pair that differs credits both labels; a pair with the outside, and p + d_k outside, credit p when border is set: a
//     closed form per voxel on an array face.  A vertex credits each distinct label around it.  The lane's own run takes its
//     credits in registers (ShAcc run); credits to other labels are merged in a second one while the label stays the same.
//   * a lane is `quiet` when its voxels and all their windows are one value and none lies on a face of the array: it joins its
//     predecessor's run with its count only (as the first lane of a wave it adds that count itself and nothing else).  A lane
//     whose voxels and windows are all background does nothing, wherever it lies.
// A slot is 136 bytes (key, count, 13 + 2 x u64), measure.hip's footprint: 256 LDS slots are 34 KiB per workgroup.  Registers
// (the five windows are kept in 32 bits per voxel unless the labels have 64): 131 / 133 VGPRs for 8- and 4-byte labels, three
// workgroups per CU; 173 / 254 for 2- and 1-byte ones, two.  The loop over a lane's voxels has to be unrolled in full or the
// windows are indexed at run time and live in scratch memory: build.py raises the size up to which `#pragma unroll` is obeyed
// for this file.  The 592 bytes of scratch per lane that remain are sh_flush's frame and its arguments: a call, to keep that
// loop short, and only lanes with something to add make it.  The Euler
// sums are signed and kept modulo 2^64, so that the overflow contract's same slab with negated weights takes out exactly what
// a failed call added.  The table around the count kernel is label_table.h's; ShapeCells tells it what a cell of this family is.
#include "common.h"
#include "label_table.h"

namespace emp {
namespace {

constexpr int SH_THREADS = 256;
constexpr int SH_LDS_SLOTS = 256;
constexpr int SH_LDS_PROBES = 8;
constexpr int SH_GLOBAL_PROBES = 128;
constexpr int64_t SH_MAX_GRID = 2048;      // two rounds of the 1024 workgroups the chip holds
constexpr uint64_t SH_EMPTY = CELL_EMPTY;  // keys lie in [0, 2^63)
constexpr int SH_DIRS = 13;
constexpr int SH_SUMS = SH_DIRS + 2;       // the intercepts, then euler closed, euler open
constexpr int SH_EULER = SH_DIRS;          // index of the first Euler sum

typedef unsigned long long ull_t;

// (dz, dy, dx) of the half-directions: first non-zero component +1, lexicographic
struct ShDirs {
  int d[SH_DIRS][3];
  constexpr ShDirs() : d() {
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
constexpr ShDirs SH_DIR;

// What a vertex adds to the two Euler numbers of a label, by the label's occupancy m of the voxels around it: bit t = 4 tz + 2 ty
// + tx is the voxel c - t (2-D: t = 2 ty + tx).  closed: a cell belongs to the label if any voxel that touches it does; the
// vertex owns itself (all 8 touch it), per axis a the edge towards c - e_a (the 4 voxels with t_a = 1), per pair of axes the
// face (the 2 voxels with both bits) and the voxel t = 7.  open: the voxel t = 7 and the pairs, quads and the octet it is the
// lowest member of, each counted when all of its voxels belong to the label.
struct ShEulerTable {
  signed char closed3[256], open3[256], closed2[16], open2[16];
  static constexpr int chi(int m, int nd, bool closed) {
    const int full = (1 << nd) - 1;
    int chi = 0;
    for (int axes = 0; axes <= full; ++axes) {      // the cell spanned by `axes` from the vertex towards lower indices
      int dim = 0, any = 0, all = 1;
      for (int a = 0; a < nd; ++a) dim += (axes >> a) & 1;
      for (int t = 0; t <= full; ++t) {
        const int in = (m >> t) & 1;
        if ((t & axes) == axes) any |= in;                  // closed: the voxels that touch the cell
        if ((t | axes) == full && !in) all = 0;             // open: the voxels of the block that voxel `full` spans along `axes`
      }
      if (closed)
        chi += ((dim & 1) ? -1 : 1) * any;
      else
        chi += ((dim & 1) ? -1 : 1) * all;
    }
    return chi;
  }
  constexpr ShEulerTable() : closed3(), open3(), closed2(), open2() {
    for (int m = 0; m < 256; ++m) {
      closed3[m] = (signed char)chi(m, 3, true);
      open3[m] = (signed char)chi(m, 3, false);
    }
    for (int m = 0; m < 16; ++m) {
      closed2[m] = (signed char)chi(m, 2, true);
      open2[m] = (signed char)chi(m, 2, false);
    }
  }
};
__constant__ ShEulerTable SH_CHI = ShEulerTable();
static_assert(ShEulerTable::chi(255, 3, true) == 0 && ShEulerTable::chi(255, 3, false) == 0 && ShEulerTable::chi(0, 3, true) == 0,
              "an interior and an empty neighbourhood add nothing");
static_assert(ShEulerTable::chi(1, 3, true) == 1 && ShEulerTable::chi(128, 3, true) == 0 && ShEulerTable::chi(128, 3, false) == 1 &&
                  ShEulerTable::chi(0x81, 3, true) == 0 && ShEulerTable::chi(0x81, 3, false) == 1 &&ShEulerTable::chi(15, 2, true) == 0 && ShEulerTable::chi(9, 2, true) == 0,
              "single voxels and a diagonal pair");

struct ShTable {
  uint64_t* hdr;
  uint64_t* keys;
  uint64_t* counts;
  uint64_t* sums;
  uint64_t mask;
};

// what a lane's run, an LDS slot or a cell adds to a cell; the Euler sums as two's complement
struct ShRec {
  uint64_t cnt;
  uint64_t s[SH_SUMS];
};

// the cell of `key`, claimed if need be; -1 and the overflow flag when the probes run out
__device__ __forceinline__ int64_t sh_global_find(const ShTable& t, uint64_t key) {
  uint64_t s = ov_hash(key) & t.mask;
#pragma unroll 1
  for (int p = 0; p < SH_GLOBAL_PROBES; ++p) {
    uint64_t cur = __hip_atomic_load(&t.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == SH_EMPTY) {
      cur = atomicCAS((ull_t*)&t.keys[s], (ull_t)SH_EMPTY, (ull_t)key);
      if (cur == SH_EMPTY) cur = key;
    }
    if (cur == key) return (int64_t)s;
    s = (s + 1) & t.mask;
  }
  atomicOr((unsigned int*)&t.hdr[1], 1u);      // dropped: the host undoes the slab and grows the table
  return -1;
}

// negate: the undo pass -- every sum with the opposite sign
__device__ __forceinline__ void sh_global_add(const ShTable& t, uint64_t key, const ShRec& r, int negate) {
  const int64_t s = sh_global_find(t, key);
  if (s < 0) return;
  if (r.cnt) atomicAdd((ull_t*)&t.counts[s], (ull_t)(negate ? 0ull - r.cnt : r.cnt));
#pragma unroll
  for (int f = 0; f < SH_SUMS; ++f)
    if (r.s[f]) atomicAdd((ull_t*)&t.sums[s * SH_SUMS + f], (ull_t)(negate ? 0ull - r.s[f] : r.s[f]));
}

struct ShCtx {
  uint64_t* lkeys;
  uint64_t* lcnt;
  uint64_t* lsum;
  ShTable t;
  uint32_t H, W, zoff, Dtot;
  float invH, invW;
  int per_slice, negate;
};

__device__ __forceinline__ int sh_lds_find(const ShCtx& c, uint64_t key) {
  uint32_t s = (uint32_t)ov_hash(key) & (SH_LDS_SLOTS - 1);
#pragma unroll 1
  for (int p = 0; p < SH_LDS_PROBES; ++p) {
    uint64_t cur = __hip_atomic_load(&c.lkeys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (cur == SH_EMPTY) {
      cur = atomicCAS((ull_t*)&c.lkeys[s], (ull_t)SH_EMPTY, (ull_t)key);
      if (cur == SH_EMPTY) cur = key;
    }
    if (cur == key) return (int)s;
    s = (s + 1) & (SH_LDS_SLOTS - 1);
  }
  return -1;
}

// what a lane has gathered for one key: the count (the run's own voxels), the intercepts and the two Euler sums
struct ShAcc {
  uint64_t key;
  uint32_t cnt;
  uint32_t n[SH_DIRS];
  int32_t e[2];
  bool live;      // something to add
};

__device__ __forceinline__ void sh_clear(ShAcc& a, uint64_t key) {
  a.key = key;
  a.cnt = 0;
#pragma unroll
  for (int k = 0; k < SH_DIRS; ++k) a.n[k] = 0;
  a.e[0] = a.e[1] = 0;
  a.live = false;
}

// the lane's sums for a.key into the workgroup's table, or into the global one when the LDS probes run out.  A call, not inlined:
// a voxel has some thirty places from which an accumulator may have to be flushed, and the loop over a lane's voxels is unrolled
__device__ __noinline__ void sh_flush(const ShCtx& c, const ShAcc a) {
  if (!a.live) return;
  const int s = sh_lds_find(c, a.key);
  if (s < 0) {
    ShRec r;
    r.cnt = a.cnt;
#pragma unroll
    for (int k = 0; k < SH_DIRS; ++k) r.s[k] = a.n[k];
    r.s[SH_EULER] = (uint64_t)(int64_t)a.e[0];
    r.s[SH_EULER + 1] = (uint64_t)(int64_t)a.e[1];
    sh_global_add(c.t, a.key, r, c.negate);
    return;
  }
  if (a.cnt) atomicAdd((ull_t*)&c.lcnt[s], (ull_t)a.cnt);
#pragma unroll
  for (int k = 0; k < SH_DIRS; ++k)
    if (a.n[k]) atomicAdd((ull_t*)&c.lsum[s * SH_SUMS + k], (ull_t)a.n[k]);
#pragma unroll
  for (int k = 0; k < 2; ++k)
    if (a.e[k]) atomicAdd((ull_t*)&c.lsum[s * SH_SUMS + SH_EULER + k], (ull_t)(int64_t)a.e[k]);
}

// A credit to `key` goes to the run's own accumulator or to the other one, which is flushed first when it holds another key:
// consecutive credits to one neighbour label are merged in registers.  One intercept along direction k ...
__device__ __forceinline__ void sh_credit_dir(const ShCtx& c, ShAcc& run, ShAcc& other, uint64_t key, int k) {
  if (key == run.key) {
    ++run.n[k];
    run.live = true;
    return;
  }
  if (other.key != key) {
    sh_flush(c, other);
    sh_clear(other, key);
  }
  ++other.n[k];
  other.live = true;
}

// ... and what a vertex adds to the two Euler sums
__device__ __forceinline__ void sh_credit_euler(const ShCtx& c, ShAcc& run, ShAcc& other, uint64_t key, int closed, int open) {
  if (key == run.key) {
    run.e[0] += closed;
    run.e[1] += open;
    run.live = true;
    return;
  }
  if (other.key != key) {
    sh_flush(c, other);
    sh_clear(other, key);
  }
  other.e[0] += closed;
  other.e[1] += open;
  other.live = true;
}

// A lane keeps its windows in 32 bits per voxel unless the labels have 64
template <int S> struct ShVal { typedef uint32_t type; };
template <> struct ShVal<8> { typedef uint64_t type; };

__device__ __forceinline__ uint32_t sh_shfl_up(uint32_t v) { return (uint32_t)__shfl_up((unsigned int)v, 1); }
__device__ __forceinline__ uint64_t sh_shfl_up(uint64_t v) { return (uint64_t)__shfl_up((ull_t)v, 1); }
__device__ __forceinline__ uint32_t sh_shfl_down(uint32_t v) { return (uint32_t)__shfl_down((unsigned int)v, 1); }
__device__ __forceinline__ uint64_t sh_shfl_down(uint64_t v) { return (uint64_t)__shfl_down((ull_t)v, 1); }

// the vertex around which the 8 (nbits = 4: the 4 of an image) voxels val[t] lie, 0 for the background and the outside: every
// distinct label among them is credited with what its occupancy gives
template <class WT>
__device__ __forceinline__ void sh_vertex(const ShCtx& c, ShAcc& run, ShAcc& other, const WT* val, uint32_t gz) {
#pragma unroll
  for (int tt = 0; tt < 8; ++tt) {
    const WT L = val[tt];
    bool first = L != 0;
    int m = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (u < tt) first &= val[u] != L;
      m |= (val[u] == L ? 1 : 0) << u;
    }
    if (first) {
      const int ec = c.per_slice ? SH_CHI.closed2[m & 15] : SH_CHI.closed3[m];
      const int eo = c.per_slice ? SH_CHI.open2[m & 15] : SH_CHI.open3[m];
      if (ec | eo) sh_credit_euler(c, run, other, c.per_slice ? ((uint64_t)gz << 32) | L : (uint64_t)L, ec, eo);
    }
  }
}

// where the windows of a lane come from: the slab (n voxels) and the slice below its first one (HW voxels, or null)
template <int S>
struct ShSrc {
  typedef typename OvElem<S>::type T;
  typedef typename ShVal<S>::type WT;
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
__device__ __forceinline__ void sh_window(const ShSrc<S>& src, int64_t s, int lane, typename ShVal<S>::type* w) {
  typedef typename OvElem<S>::type T;
  typedef typename OvVec<S * E>::type V;
  typedef typename ShVal<S>::type WT;
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
  w[0] = sh_shfl_up(w[E]);
  w[E + 1] = sh_shfl_down(w[1]);
  if (lane == 0) w[0] = src.at(s - 1);
  if (lane == 63) w[E + 1] = src.at(s + E);
}

// a: the slab (n voxels); halo: the slice below its first one (H * W voxels) or null; zoff: the slab's first slice, Dtot: the
// volume's depth
template <int S>
__global__ void __launch_bounds__(SH_THREADS) label_shape_kernel(const void* __restrict__ a, const void* __restrict__ halo, int64_t n,
                                                                 int is_signed, int64_t tiles_per_wg, ShTable t, uint32_t H, uint32_t W,
                                                                 uint32_t zoff, uint32_t Dtot, float invH, float invW, int per_slice, int border,
                                                                 int negate) {
  typedef typename OvElem<S>::type T;
  typedef typename ShVal<S>::type WT;
  constexpr int E = 16 / S;
  constexpr uint32_t TILE = SH_THREADS * E;
  __shared__ uint64_t lkeys[SH_LDS_SLOTS];
  __shared__ uint64_t lcnt[SH_LDS_SLOTS];
  __shared__ uint64_t lsum[SH_LDS_SLOTS * SH_SUMS];
  for (int i = threadIdx.x; i < SH_LDS_SLOTS; i += SH_THREADS) {
    lkeys[i] = SH_EMPTY;
    lcnt[i] = 0;
#pragma unroll
    for (int f = 0; f < SH_SUMS; ++f) lsum[i * SH_SUMS + f] = 0;
  }
  __syncthreads();
  ShCtx c;
  c.lkeys = lkeys;
  c.lcnt = lcnt;
  c.lsum = lsum;
  c.t = t;
  c.H = H;
  c.W = W;
  c.zoff = zoff;
  c.Dtot = Dtot;
  c.invH = invH;
  c.invW = invW;
  c.per_slice = per_slice;
  c.negate = negate;
  const int lane = threadIdx.x & 63;
  ShSrc<S> src;
  src.a = (const T*)a;
  src.halo = (const T*)halo;
  src.n = n;
  src.HW = (int64_t)H * W;
  const int64_t HW = src.HW;
  const uint32_t bf = border ? 1u : 0u;
  const int ndirs = per_slice ? 4 : SH_DIRS;
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
    sh_window<S, E>(src, i0, lane, win[0]);
    sh_window<S, E>(src, i0 - (int64_t)W, lane, win[1]);
    if (!per_slice) {
      sh_window<S, E>(src, i0 - HW + (int64_t)W, lane, win[2]);
      sh_window<S, E>(src, i0 - HW, lane, win[3]);
      sh_window<S, E>(src, i0 - HW - (int64_t)W, lane, win[4]);
    }
    const WT* v = &win[0][1];
    uint32_t x, y, z;
    ov_coord(c, bx, by, bz, o0, x, y, z);
    bool uni = nv == E, same = win[0][0] == v[0];
#pragma unroll
    for (int j = 0; j < E; ++j) {
      bad = bad || (j < nv && ov_key_out_of_range<S>(v[j], is_signed, per_slice));
      uni &= v[j] == v[0];
    }
#pragma unroll
    for (int j = 0; j < E + 2; ++j) {
      same &= win[1][j] == v[0];
      if (!per_slice) same &= win[2][j] == v[0] && win[3][j] == v[0] && win[4][j] == v[0];
    }
    bool flat = same;      // the voxels the lane holds (those beyond the slab read as 0) and all their windows are one value
#pragma unroll
    for (int j = 0; j < E; ++j) flat &= v[j] == v[0];
    const bool blank = flat && v[0] == 0;      // background all around: nothing to count, on a face of the array or not
    // quiet: one value in the lane and all around it, and no voxel on a face of the array -- no intercept, no vertex, no row end
    const bool quiet = uni && same && x > 0 && x + E < W && y > 0 && y + 1 < H && (per_slice || (zoff + z > 0 && zoff + z + 1 < Dtot));
    // a quiet lane continues the run of a uniform predecessor with the same label
    const WT prev_v = sh_shfl_up(v[0]);
    const int prev_uni = __shfl_up((int)uni, 1);
    const bool head = !quiet || lane == 0 || !prev_uni || prev_v != v[0];
    const uint64_t heads = __ballot(head);
    if (head && nv > 0 && !blank) {
      uint32_t ext = 0;      // voxels of the quiet lanes that follow a uniform head
      if (uni) {
        const uint64_t above = lane == 63 ? 0ull : heads >> (lane + 1);
        const int lanes = above ? __ffsll((ull_t)above) : 64 - lane;
        ext = (uint32_t)(lanes - 1) * E;
      }
      ShAcc run, other;
      sh_clear(run, per_slice ? ((uint64_t)(zoff + z) << 32) | v[0] : (uint64_t)v[0]);
      sh_clear(other, SH_EMPTY);
      WT cur = v[0];
      if (quiet) {      // the first lane of a wave inside an object: its voxels' count (and its followers'), nothing else
        run.cnt = E;
        run.live = cur != 0;
      }
#pragma unroll
      for (int j = 0; j < E; ++j) {
        if (quiet) break;
        if (j < nv) {
          const uint32_t gz = zoff + z;
          const WT own = v[j];
          if (j > 0 && (own != cur || (per_slice && x == 0 && y == 0))) {      // the run ends (per slice: also where the key changes)
            if (cur != 0) sh_flush(c, run);
            cur = own;
            sh_clear(run, per_slice ? ((uint64_t)gz << 32) | own : (uint64_t)own);
          }
          if (own != 0) {
            ++run.cnt;
            run.live = true;
          }
          // which neighbours exist: low[a] the one at index - 1, high[a] the one at index + 1 of axis a (z, y, x)
          const bool low[3] = {!per_slice && gz > 0, y > 0, x > 0};
          const bool high[3] = {!per_slice && gz + 1 < Dtot, y + 1 < H, x + 1 < W};
          // the 13 pairs (p - d_k, p), and what p + d_k outside the array adds
#pragma unroll
          for (int k = 0; k < SH_DIRS; ++k) {
            if (k < ndirs) {
              const int dz = SH_DIR.d[k][0], dy = SH_DIR.d[k][1], dx = SH_DIR.d[k][2];
              // p - d: dz, dy, dx = 1 step to the lower index, -1 to the higher one
              const bool inside = (dz == 0 || low[0]) && (dy == 0 || (dy > 0 ? low[1] : high[1])) && (dx == 0 || (dx > 0 ? low[2] : high[2]));
              const bool beyond = (dz == 0 || high[0]) && (dy == 0 || (dy > 0 ? high[1] : low[1])) && (dx == 0 || (dx > 0 ? high[2] : low[2]));
              const WT nb = win[dz ? 3 + dy : dy][1 + j - dx];
              const uint32_t mine = (inside ? (nb != own ? 1u : 0u) : bf) + (beyond ? 0u : bf);
              if (own != 0) {
                run.n[k] += mine;
                run.live |= mine != 0;
              }
              if (inside && nb != own && nb != 0) sh_credit_dir(c, run, other, per_slice ? ((uint64_t)gz << 32) | nb : (uint64_t)nb, k);
            }
          }
          // the vertices: c = p, and c = p + e for every e in {0, 1}^3 whose axes have p at their last index
          WT o[8];      // o[t] = the voxel p - t, 0 outside the array
#pragma unroll
          for (int tt = 0; tt < 8; ++tt) {
            const int tz = tt >> 2, ty = (tt >> 1) & 1, tx = tt & 1;
            const bool inside = (!tz || low[0]) && (!ty || low[1]) && (!tx || low[2]);      // low[0] is never set per slice
            o[tt] = inside ? win[tz ? 3 + ty : ty][1 + j - tx] : (WT)0;
          }
          bool plain = true;      // one value around the vertex c = p: it adds nothing
#pragma unroll
          for (int tt = 1; tt < 8; ++tt) plain &= (per_slice && tt >= 4) || o[tt] == own;
          if (!plain) sh_vertex<WT>(c, run, other, o, gz);
          const int last = (!per_slice && gz + 1 == Dtot ? 4 : 0) | (y + 1 == H ? 2 : 0) | (x + 1 == W ? 1 : 0);
          if (last) {      // rare: the one place where the voxels around a vertex are picked by a run-time index
            WT oo[8];
#pragma unroll
            for (int tt = 0; tt < 8; ++tt) oo[tt] = o[tt];
#pragma unroll 1
            for (int e = 1; e < 8; ++e) {
              if ((e & last) != e) continue;
              WT val[8];      // the voxel c - t = p - (t - e); an axis of e with t = 0 is the outside
#pragma unroll
              for (int tt = 0; tt < 8; ++tt) val[tt] = (e & ~tt) != 0 ? (WT)0 : oo[tt ^ e];
              sh_vertex<WT>(c, run, other, val, gz);
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
      if (cur != 0) {
        run.cnt += ext;
        sh_flush(c, run);
      }
      sh_flush(c, other);
    }
    ov_coord(c, bx, by, bz, TILE, bx, by, bz);
  }
  if (bad) atomicOr((unsigned int*)&t.hdr[1] + 1, 1u);
  __syncthreads();
  for (int i = threadIdx.x; i < SH_LDS_SLOTS; i += SH_THREADS) {
    const uint64_t k = lkeys[i];
    if (k == SH_EMPTY) continue;
    ShRec r;
    r.cnt = lcnt[i];
    bool any = r.cnt != 0;
#pragma unroll
    for (int f = 0; f < SH_SUMS; ++f) {
      r.s[f] = lsum[i * SH_SUMS + f];
      any |= r.s[f] != 0;
    }
    if (any) sh_global_add(t, k, r, negate);
  }
}

// a cell is a key, a count and SH_SUMS x u64; finalize gives the intercepts and the Euler numbers as two columns
struct ShapeCells {
  typedef ShTable Table;
  struct Out {
    uint64_t* keys;
    uint64_t* counts;
    uint64_t* intercepts;
    int64_t* euler;
  };
  static constexpr size_t SLOT_BYTES = 16 + 8 * SH_SUMS;
  static constexpr int HEADER_CELLS = 0;
  static void layout(ShTable& t, int64_t capacity) { t.sums = t.counts + capacity; }
  static __device__ void clear(const ShTable& t, int64_t i) {
    for (int f = 0; f < SH_SUMS; ++f) t.sums[i * SH_SUMS + f] = 0;
  }
  static __device__ void move(const ShTable& from, int64_t i, uint64_t k, uint64_t w, const ShTable& to) {
    ShRec r;
    r.cnt = w;
    for (int f = 0; f < SH_SUMS; ++f) r.s[f] = from.sums[i * SH_SUMS + f];
    sh_global_add(to, k, r, 0);
  }
  static __device__ void write(const ShTable& t, int64_t i, const Out& out, int64_t pos) {
    for (int f = 0; f < SH_DIRS; ++f) out.intercepts[pos * SH_DIRS + f] = t.sums[i * SH_SUMS + f];
    for (int f = 0; f < 2; ++f) out.euler[pos * 2 + f] = (int64_t)t.sums[i * SH_SUMS + SH_EULER + f];
  }
};
static_assert(ShapeCells::SLOT_BYTES == 136, "measure.hip's footprint");

struct ShSlab {
  const void* a;
  const void* halo;
  int64_t n, z0, D;
  int H, W, per_slice, border;
};

template <int S>
int sh_launch(const ShSlab& g, int is_signed, const ShTable& t, int negate, hipStream_t s) {
  constexpr int64_t TILE = (int64_t)SH_THREADS * (16 / S);
  const int64_t ntiles = (g.n + TILE - 1) / TILE;
  const int64_t per = (ntiles + SH_MAX_GRID - 1) / SH_MAX_GRID;
  const int grid = (int)((ntiles + per - 1) / per);
  hipLaunchKernelGGL((label_shape_kernel<S>), dim3(grid), dim3(SH_THREADS), 0, s, g.a, g.halo, g.n, is_signed, per, t, (uint32_t)g.H,
                     (uint32_t)g.W, (uint32_t)g.z0, (uint32_t)g.D, 1.0f / (float)g.H, 1.0f / (float)g.W, g.per_slice, g.border, negate);
  EMP_LAUNCH_CHECK();
  return EMP_OK;
}

int sh_dispatch(const ShSlab& g, int in_bytes, const ShTable& t, int negate, hipStream_t s) {
  const int sg = in_bytes < 0, A = sg ? -in_bytes : in_bytes;
  if (A == 1) return sh_launch<1>(g, sg, t, negate, s);
  if (A == 2) return sh_launch<2>(g, sg, t, negate, s);
  if (A == 4) return sh_launch<4>(g, sg, t, negate, s);
  if (A == 8) return sh_launch<8>(g, sg, t, negate, s);
  set_error("label_shape: element size %d unsupported (1, 2, 4, 8; negative = signed)", in_bytes);
  return EMP_ERR_INVALID;
}

}  // namespace
}  // namespace emp

using namespace emp;

extern "C" {

size_t emp_label_shape_work_bytes(int64_t capacity) {
  return cells_capacity_ok(capacity) ? CELL_HEADER + (size_t)capacity * ShapeCells::SLOT_BYTES : 0;
}

int emp_label_shape_reset(void* d_table, int64_t capacity, void* stream) {
  EMP_REQUIRE(d_table && cells_capacity_ok(capacity), "label_shape_reset: the capacity must be a power of two in [64, 2^32]");
  return cells_reset<ShapeCells>(d_table, capacity, (hipStream_t)stream);
}

// Synchronises the stream (it reads the table's flags).  *h_overflow = 1: the table was too small for this slab; what the call
// had added has been taken out again.
int emp_label_shape_accumulate(const void* d_labels, int in_bytes, int64_t z0, int depth, int H, int W, int64_t total_depth,
                               const void* d_halo, int per_slice, int border_faces, void* d_table, int64_t capacity, void* stream,
                               int* h_overflow) {
  EMP_REQUIRE(d_table && cells_capacity_ok(capacity) && h_overflow && depth >= 0 && H > 0 && W > 0 && (depth == 0 || d_labels),
              "label_shape_accumulate: bad arguments");
  EMP_REQUIRE(z0 >= 0 && total_depth >= z0 + depth, "label_shape_accumulate: the slab [%lld, %lld) does not lie in a volume of depth %lld",
              (long long)z0, (long long)(z0 + depth), (long long)total_depth);
  EMP_REQUIRE(total_depth < (1ll << 31) && H < (1 << 30) && W < (1 << 30), "label_shape_accumulate: shape (%lld, %d, %d) beyond 2^31, 2^30, 2^30",
              (long long)total_depth, H, W);
  per_slice = per_slice != 0;
  EMP_REQUIRE(per_slice || z0 == 0 || depth == 0 || d_halo, "label_shape_accumulate: a slab that starts at slice %lld needs the slice below it (d_halo)",
              (long long)z0);
  hipStream_t s = (hipStream_t)stream;
  *h_overflow = 0;
  ShSlab g;
  g.a = d_labels;
  g.halo = (per_slice || z0 == 0) ? nullptr : d_halo;
  g.n = (int64_t)depth * H * W;
  g.z0 = z0;
  g.D = total_depth;
  g.H = H;
  g.W = W;
  g.per_slice = per_slice;
  g.border = border_faces != 0;
  if (g.n == 0) return EMP_OK;
  const ShTable t = cells_table<ShapeCells>(d_table, capacity);
  return cells_accumulate(t.hdr, s, "label_shape_accumulate", "the key's domain (negative, or beyond 2^63 / per slice 2^32)",
                          [&](int negate) { return sh_dispatch(g, in_bytes, t, negate, s); }, h_overflow);
}

// Moves the cells of a table into an empty (reset) larger one.  Synchronises; *h_overflow = 1: d_to is too small as well.
int emp_label_shape_grow(const void* d_from, int64_t from_capacity, void* d_to, int64_t to_capacity, void* stream, int* h_overflow) {
  EMP_REQUIRE(d_from && d_to && cells_capacity_ok(from_capacity) && cells_capacity_ok(to_capacity) && to_capacity > from_capacity && h_overflow,
              "label_shape_grow: bad arguments");
  return cells_grow<ShapeCells>(d_from, from_capacity, d_to, to_capacity, (hipStream_t)stream, h_overflow);
}

// Synchronises.  *h_num = number of keys; the first min(*h_num, max_out) of them are written.
int emp_label_shape_finalize(void* d_table, int64_t capacity, uint64_t* d_keys, uint64_t* d_counts, uint64_t* d_intercepts, int64_t* d_euler,
                             int64_t max_out, int64_t* h_num, void* stream) {
  EMP_REQUIRE(d_table && cells_capacity_ok(capacity) && h_num && max_out >= 0 && (max_out == 0 || (d_keys && d_counts && d_intercepts && d_euler)),
              "label_shape_finalize: bad arguments");
  return cells_finalize<ShapeCells>(d_table, capacity, {d_keys, d_counts, d_intercepts, d_euler}, max_out, h_num, (hipStream_t)stream);
}

}  // extern "C"
