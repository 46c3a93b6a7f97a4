// Measure Labels on the device: per label that occurs (0, the background, excepted) the voxel count, the bounding box, the raw
// first and second moments of the voxel coordinates and the number of exposed voxel faces per axis -- what
// regionprops_table(img, properties=('label', 'area', 'bbox', 'centroid', 'moments', 'inertia_tensor', 'perimeter')) is asked for
// after a segmentation.  skimage is not available where this library is built: area (voxel count), bbox (min and exclusive max
// per axis), centroid (mean index coordinate) and the raw moments sum z^a y^b x^c are restated from their documented behaviour,
// not pinned against them; the face count is this library's own statement of a surface (skimage's `perimeter` is a weighted
// boundary-pixel count and is not reproduced).  Everything is an integer, so the result is exact and does not depend on how the
// volume is cut into slabs.
//
// One kernel per slab.  It follows label_table_kernel (labels.hip): 16-byte loads, one vector per lane; a tile's first voxel
// is carried along the workgroup's stretch of tiles; a bounded-probe LDS table per workgroup, flushed with one global update
// per occupied slot.  What differs:
//   * moments come from runs in closed form.  A run is an interval of the raveled slab; it is cut into at most five boxes
//     (the rest of its first row, the rest of its first slice, whole slices, the head of its last slice, the head of its last
//     row), and a box [z0, z1] x [y0, y1] x [x0, x1] adds sum x = nz ny (x0 + x1) nx / 2, sum x^2 by the square-pyramid
//     formula, sum yx = nz (sum y)(sum x) and so on.  The sums of a run are formed in registers and enter LDS once.
//   * faces need the voxel's -x, -y and -z neighbours: one more (mostly unaligned) read of the rows above and of the slice
//     below, the latter from the halo slice for the slab's first slice.  A pair that differs credits both of its labels; the
//     first and last index of an axis credit against the outside when border_faces is set.  A lane adds its own voxels' faces
//     to the run they belong to, and merges consecutive credits to one neighbour label before it touches LDS.
//   * a lane is `quiet` when its voxels and all their neighbours are one value and none lies on a face of the array: it has no
//     faces, and joins its predecessor's run as a uniform lane does in label_table_kernel.  Uniform background costs the loads
//     and the compares and nothing else: label 0 is never entered.
// A slot is 136 bytes (key, count, 6 x u32 box, 12 x u64 sums).  256 LDS slots are 34 KiB per workgroup: four workgroups of
// 256 threads per CU in 136 of its 160 KiB.  Registers allow as many for 4- and 8-byte labels (113 / 101 VGPRs); the three
// neighbour vectors of 8 and 16 elements leave three workgroups per CU for 2-byte labels (149) and two for 1-byte ones (199).
// Overflow: as in labels.hip, slots are never released; the same slab with negated weights takes out exactly what a failed call
// added (every sum and face count is an add modulo 2^64); box fields are idempotent and are not undone.  A cell can hold face
// credits from the slab above it before its own count arrives; cells whose count is 0 do not exist for grow / finalize.
// The table around the count kernel -- layout, reset, rehash, compaction, the host side of accumulate / grow / finalize -- is
// label_table.h's; MeasureCells below tells it what a cell of this family is.
#include "common.h"
#include "label_table.h"

namespace emp {
namespace {

constexpr int MZ_THREADS = 256;
constexpr int MZ_LDS_SLOTS = 256;
constexpr int MZ_LDS_PROBES = 8;
constexpr int MZ_GLOBAL_PROBES = 128;
constexpr int64_t MZ_MAX_GRID = 2048;      // two rounds of the 1024 workgroups the chip holds
constexpr uint64_t MZ_EMPTY = CELL_EMPTY;  // keys lie in [0, 2^63)
constexpr int MZ_SUMS = 12;                // sum z, y, x; sum zz, yy, xx, zy, zx, yx; faces z, y, x
constexpr int MZ_FACES = 9;                // index of the first face count

typedef unsigned long long ull_t;

struct MzTable {
  uint64_t* hdr;
  uint64_t* keys;
  uint64_t* counts;
  uint64_t* sums;
  uint32_t* box;
  uint64_t mask;
};

// what a run, an LDS slot or a cell adds to a cell
struct MzRec {
  uint64_t cnt;
  uint64_t s[MZ_SUMS];
  uint32_t lo[3], hi[3];      // z, y, x; inclusive
};

// the cell of `key`, claimed if need be; -1 and the overflow flag when the probes run out
__device__ __forceinline__ int64_t mz_global_find(const MzTable& t, uint64_t key) {
  uint64_t s = ov_hash(key) & t.mask;
#pragma unroll 1
  for (int p = 0; p < MZ_GLOBAL_PROBES; ++p) {
    uint64_t cur = __hip_atomic_load(&t.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == MZ_EMPTY) {
      cur = atomicCAS((ull_t*)&t.keys[s], (ull_t)MZ_EMPTY, (ull_t)key);
      if (cur == MZ_EMPTY) cur = key;
    }
    if (cur == key) return (int64_t)s;
    s = (s + 1) & t.mask;
  }
  atomicOr((unsigned int*)&t.hdr[1], 1u);      // dropped: the host undoes the slab and grows the table
  return -1;
}

// negate: the undo pass -- sums and counts with the opposite sign, the box left alone
__device__ __forceinline__ void mz_global_add(const MzTable& t, uint64_t key, const MzRec& r, int negate) {
  const int64_t s = mz_global_find(t, key);
  if (s < 0) return;
  if (r.cnt) atomicAdd((ull_t*)&t.counts[s], (ull_t)(negate ? 0ull - r.cnt : r.cnt));
#pragma unroll
  for (int f = 0; f < MZ_SUMS; ++f)
    if (r.s[f]) atomicAdd((ull_t*)&t.sums[s * MZ_SUMS + f], (ull_t)(negate ? 0ull - r.s[f] : r.s[f]));
  if (!negate && r.cnt) ov_box_update_global(&t.box[s * 6], r);
}

struct MzCtx {
  uint64_t* lkeys;
  uint64_t* lcnt;
  uint64_t* lsum;
  uint32_t* lbox;
  MzTable t;
  uint32_t H, W, zoff, Dtot;
  float invH, invW;
  int per_slice, negate;
};

__device__ __forceinline__ int mz_lds_find(const MzCtx& c, uint64_t key) {
  uint32_t s = (uint32_t)ov_hash(key) & (MZ_LDS_SLOTS - 1);
#pragma unroll 1
  for (int p = 0; p < MZ_LDS_PROBES; ++p) {
    uint64_t cur = __hip_atomic_load(&c.lkeys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (cur == MZ_EMPTY) {
      cur = atomicCAS((ull_t*)&c.lkeys[s], (ull_t)MZ_EMPTY, (ull_t)key);
      if (cur == MZ_EMPTY) cur = key;
    }
    if (cur == key) return (int)s;
    s = (s + 1) & (MZ_LDS_SLOTS - 1);
  }
  return -1;
}

__device__ __forceinline__ void mz_add(const MzCtx& c, uint64_t key, const MzRec& r) {
  const int s = mz_lds_find(c, key);
  if (s < 0) {
    mz_global_add(c.t, key, r, c.negate);
    return;
  }
  if (r.cnt) atomicAdd((ull_t*)&c.lcnt[s], (ull_t)r.cnt);
#pragma unroll
  for (int f = 0; f < MZ_SUMS; ++f)
    if (r.s[f]) atomicAdd((ull_t*)&c.lsum[s * MZ_SUMS + f], (ull_t)r.s[f]);
  if (!c.negate && r.cnt) {
    uint32_t* b = &c.lbox[s * 6];
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      if (r.lo[f] < __hip_atomic_load(&b[f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) atomicMin(&b[f], r.lo[f]);
      if (r.hi[f] > __hip_atomic_load(&b[3 + f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) atomicMax(&b[3 + f], r.hi[f]);
    }
  }
}

// n faces perpendicular to `axis` for a label met as a neighbour (its voxels are counted by the lane, or the slab, that holds them)
__device__ __forceinline__ void mz_credit(const MzCtx& c, uint64_t key, int axis, uint32_t n) {
  const int s = mz_lds_find(c, key);
  if (s >= 0) {
    atomicAdd((ull_t*)&c.lsum[s * MZ_SUMS + MZ_FACES + axis], (ull_t)n);
    return;
  }
  const int64_t g = mz_global_find(c.t, key);
  if (g >= 0) atomicAdd((ull_t*)&c.t.sums[g * MZ_SUMS + MZ_FACES + axis], (ull_t)(c.negate ? 0ull - n : (uint64_t)n));
}

// consecutive credits to one neighbour label along one axis, merged in registers
struct MzNeighbour {
  uint64_t key;
  uint32_t n;
};

__device__ __forceinline__ void mz_neighbour(const MzCtx& c, MzNeighbour& a, uint64_t label, uint32_t gz, int axis) {
  if (label == 0) return;
  const uint64_t key = c.per_slice ? ((uint64_t)gz << 32) | label : label;
  if (a.n && a.key != key) {
    mz_credit(c, a.key, axis, a.n);
    a.n = 0;
  }
  a.key = key;
  ++a.n;
}

// sum of i and of i^2 over [a, b], b < 2^21.  Coordinates and lengths stay 32-bit so that a product is one 32 x 32 -> 64
// multiply wherever both factors allow it: the head of a run is multiplies more than anything else
__device__ __forceinline__ uint64_t mz_sum1(uint32_t a, uint32_t b) { return (uint64_t)(a + b) * (b - a + 1) / 2; }
__device__ __forceinline__ uint64_t mz_pyramid(uint32_t n) { return (uint64_t)n * (n + 1) / 2 * (2 * n + 1) / 3; }
__device__ __forceinline__ uint64_t mz_sum2(uint32_t a, uint32_t b) { return mz_pyramid(b) - (a ? mz_pyramid(a - 1) : 0ull); }

// the voxels [x0, x1] of row (z, y)
__device__ __forceinline__ void mz_row(MzRec& r, uint32_t z, uint32_t y, uint32_t x0, uint32_t x1) {
  const uint32_t n = x1 - x0 + 1;
  const uint64_t sx = mz_sum1(x0, x1), zn = (uint64_t)z * n, yn = (uint64_t)y * n;
  r.cnt += n;
  r.s[0] += zn;
  r.s[1] += yn;
  r.s[2] += sx;
  r.s[3] += zn * z;
  r.s[4] += yn * y;
  r.s[5] += mz_sum2(x0, x1);
  r.s[6] += zn * y;
  r.s[7] += sx * z;
  r.s[8] += sx * y;
}

// the rows [y0, y1] of the slices [z0, z1], whole width
__device__ __forceinline__ void mz_rows(MzRec& r, uint32_t z0, uint32_t z1, uint32_t y0, uint32_t y1, uint32_t W) {
  const uint64_t nz = z1 - z0 + 1, ny = y1 - y0 + 1;
  const uint64_t sz = mz_sum1(z0, z1), sy = mz_sum1(y0, y1), sx = mz_sum1(0, W - 1);
  r.cnt += nz * ny * W;
  r.s[0] += sz * ny * W;
  r.s[1] += sy * nz * W;
  r.s[2] += sx * nz * ny;
  r.s[3] += mz_sum2(z0, z1) * ny * W;
  r.s[4] += mz_sum2(y0, y1) * nz * W;
  r.s[5] += mz_sum2(0, W - 1) * nz * ny;
  r.s[6] += sz * sy * W;
  r.s[7] += sz * sx * ny;
  r.s[8] += sy * sx * nz;
}

// a run of len (<= 2^10) voxels of `label` that starts at the slab's voxel (zs, ys, xs), with the faces f[z, y, x] its lane
// counted for it (they belong to voxels of the run's first slice): one entry, or one per slice in per-slice mode
__device__ __forceinline__ void mz_run(const MzCtx& c, uint64_t label, uint32_t xs, uint32_t ys, uint32_t zs, uint32_t len, const uint32_t* f) {
  if (label == 0) return;
  uint32_t xe, ye, ze;
  ov_coord(c, xs, ys, zs, len - 1, xe, ye, ze);
  const uint32_t W = c.W, H = c.H;
  for (uint32_t z = zs;; ++z) {
    const uint32_t zl = c.per_slice ? z : ze;      // the entry covers the slices z .. zl
    const bool first = z == zs, last = zl == ze;
    const uint32_t y0 = first ? ys : 0u, x0 = first ? xs : 0u, y1 = last ? ye : c.H - 1, x1 = last ? xe : c.W - 1;
    const uint32_t g0 = c.zoff + z, g1 = c.zoff + zl;
    MzRec r;
    r.cnt = 0;
#pragma unroll
    for (int i = 0; i < MZ_SUMS; ++i) r.s[i] = 0;
    if (z == zl && y0 == y1) {
      mz_row(r, g0, y0, x0, x1);
    } else {
      mz_row(r, g0, y0, x0, W - 1);
      mz_row(r, g1, y1, 0, x1);
      if (z == zl) {
        if (y0 + 1 < y1) mz_rows(r, g0, g0, y0 + 1, y1 - 1, W);
      } else {
        if (y0 + 1 < H) mz_rows(r, g0, g0, y0 + 1, H - 1, W);
        if (z + 1 < zl) mz_rows(r, g0 + 1, g1 - 1, 0, H - 1, W);
        if (y1 > 0) mz_rows(r, g1, g1, 0, y1 - 1, W);
      }
    }
    if (first) {
#pragma unroll
      for (int a = 0; a < 3; ++a) r.s[MZ_FACES + a] = f[a];
    }
    const bool multi = z != zl, rows = multi || y0 != y1;
    r.lo[0] = g0;
    r.hi[0] = g1;
    r.lo[1] = multi ? 0u : y0;
    r.hi[1] = multi ? c.H - 1 : y1;
    r.lo[2] = rows ? 0u : x0;
    r.hi[2] = rows ? c.W - 1 : x1;
    mz_add(c, c.per_slice ? ((uint64_t)g0 << 32) | label : label, r);
    if (last) break;
  }
}

// E elements from element i0 of `base` on, of which those with an index in [0, ..) and j < nv exist (the rest read as 0):
// one vector load where the address allows it
template <int S, int E>
__device__ __forceinline__ void mz_load(const void* base, int64_t i0, int nv, uint64_t* v) {
  typedef typename OvElem<S>::type T;
  typedef typename OvVec<S * E>::type V;
  const T* p = (const T*)base + i0;
  if (i0 >= 0 && nv == E && (uintptr_t)p % (S * E) == 0) {
    ov_unpack<S, E>(*(const V*)p, v);
  } else {
#pragma unroll
    for (int j = 0; j < E; ++j) v[j] = (j < nv && i0 + j >= 0) ? (uint64_t)p[j] : 0ull;
  }
}

// a: the slab (n voxels); halo: the slice below its first one (H * W voxels) or null; zoff: the slab's first slice, Dtot: the
// volume's depth
template <int S>
__global__ void __launch_bounds__(MZ_THREADS) label_measure_kernel(const void* __restrict__ a, const void* __restrict__ halo, int64_t n,
                                                                   int is_signed, int64_t tiles_per_wg, MzTable t, uint32_t H, uint32_t W,
                                                                   uint32_t zoff, uint32_t Dtot, float invH, float invW, int per_slice,
                                                                   int border, int negate) {
  typedef typename OvElem<S>::type T;
  constexpr int E = 16 / S;
  constexpr uint32_t TILE = MZ_THREADS * E;
  __shared__ uint64_t lkeys[MZ_LDS_SLOTS];
  __shared__ uint64_t lcnt[MZ_LDS_SLOTS];
  __shared__ uint64_t lsum[MZ_LDS_SLOTS * MZ_SUMS];
  __shared__ uint32_t lbox[MZ_LDS_SLOTS * 6];
  for (int i = threadIdx.x; i < MZ_LDS_SLOTS; i += MZ_THREADS) {
    lkeys[i] = MZ_EMPTY;
    lcnt[i] = 0;
#pragma unroll
    for (int f = 0; f < MZ_SUMS; ++f) lsum[i * MZ_SUMS + f] = 0;
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      lbox[i * 6 + f] = 0xffffffffu;
      lbox[i * 6 + 3 + f] = 0u;
    }
  }
  __syncthreads();
  MzCtx c;
  c.lkeys = lkeys;
  c.lcnt = lcnt;
  c.lsum = lsum;
  c.lbox = lbox;
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
  const int64_t HW = (int64_t)H * W;
  const uint32_t bf = border ? 1u : 0u;
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
    uint64_t v[E], up[E], below[E];
    mz_load<S, E>(a, i0, nv, v);
    mz_load<S, E>(a, i0 - (int64_t)W, nv, up);
    if (per_slice) {
#pragma unroll
      for (int j = 0; j < E; ++j) below[j] = 0;
    } else if (i0 >= HW) {
      mz_load<S, E>(a, i0 - HW, nv, below);
    } else if (i0 + E <= HW) {
      mz_load<S, E>(halo, i0, halo ? nv : 0, below);
    } else {      // the lane straddles the end of the slab's first slice
#pragma unroll
      for (int j = 0; j < E; ++j) {
        const int64_t i = i0 + j;
        below[j] = j >= nv ? 0ull : (i >= HW ? (uint64_t)((const T*)a)[i - HW] : (halo ? (uint64_t)((const T*)halo)[i] : 0ull));
      }
    }
    // the voxel before the lane's first: the predecessor's last, or a load for the wave's first lane
    uint64_t before = (uint64_t)__shfl_up((ull_t)v[E - 1], 1);
    if (lane == 0) before = (i0 > 0 && nv > 0) ? (uint64_t)((const T*)a)[i0 - 1] : 0ull;
    uint32_t x, y, z;
    ov_coord(c, bx, by, bz, o0, x, y, z);
    const uint32_t gz = zoff + z;
    bool uni = nv == E, same = before == v[0];
#pragma unroll
    for (int j = 0; j < E; ++j) {
      bad = bad || ov_key_out_of_range<S>(v[j], is_signed, per_slice);
      uni &= v[j] == v[0];
      same &= up[j] == v[0] && (per_slice || below[j] == v[0]);
    }
    // quiet: one value in the lane and all around it, and no voxel on a face of the array -- no faces, no row end
    const bool quiet = uni && same && x > 0 && x + E < W && y > 0 && y + 1 < H && (per_slice || (gz > 0 && gz + 1 < Dtot));
    // a quiet lane continues the run of a uniform predecessor with the same label
    const uint64_t prev_v = (uint64_t)__shfl_up((ull_t)v[0], 1);
    const int prev_uni = __shfl_up((int)uni, 1);
    const bool head = !quiet || lane == 0 || !prev_uni || prev_v != v[0];
    const uint64_t heads = __ballot(head);
    if (head && nv > 0) {
      uint32_t ext = 0;      // voxels of the quiet lanes that follow a uniform head
      if (uni) {
        const uint64_t above = lane == 63 ? 0ull : heads >> (lane + 1);
        const int lanes = above ? __ffsll((ull_t)above) : 64 - lane;
        ext = (uint32_t)(lanes - 1) * E;
      }
      MzNeighbour ny, nz;
      ny.n = nz.n = 0;
      ny.key = nz.key = 0;
      uint64_t cur = v[0];
      uint32_t rx = x, ry = y, rz = z, len = 0, f[3] = {0, 0, 0};
#pragma unroll
      for (int j = 0; j < E; ++j) {
        if (j < nv) {
          const uint64_t lft = j ? v[j - 1] : before;
          const bool differs = x > 0 && lft != v[j];
          if (j > 0 && (v[j] != cur || (per_slice && x == 0 && y == 0))) {      // the run ends (per slice: also where the key changes)
            f[2] += differs;
            mz_run(c, cur, rx, ry, rz, len, f);
            cur = v[j];
            rx = x;
            ry = y;
            rz = z;
            len = 0;
            f[0] = f[1] = f[2] = 0;
          } else if (j == 0 && differs && before != 0) {      // the voxel before belongs to another lane's run
            mz_credit(c, per_slice ? ((uint64_t)(zoff + z) << 32) | before : before, 2, 1);
          }
          ++len;
          f[2] += differs + (x == 0 ? bf : 0u) + (x + 1 == W ? bf : 0u);
          if (y > 0 && up[j] != v[j]) {
            ++f[1];
            mz_neighbour(c, ny, up[j], zoff + z, 1);
          }
          f[1] += (y == 0 ? bf : 0u) + (y + 1 == H ? bf : 0u);
          if (!per_slice) {
            const uint32_t g = zoff + z;
            if (g > 0 && (z > 0 || halo) && below[j] != v[j]) {
              ++f[0];
              mz_neighbour(c, nz, below[j], g, 0);
            }
            f[0] += (g == 0 ? bf : 0u) + (g + 1 == Dtot ? bf : 0u);
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
      mz_run(c, cur, rx, ry, rz, len + ext, f);
      if (ny.n) mz_credit(c, ny.key, 1, ny.n);
      if (nz.n) mz_credit(c, nz.key, 0, nz.n);
    }
    ov_coord(c, bx, by, bz, TILE, bx, by, bz);
  }
  if (bad) atomicOr((unsigned int*)&t.hdr[1] + 1, 1u);
  __syncthreads();
  for (int i = threadIdx.x; i < MZ_LDS_SLOTS; i += MZ_THREADS) {
    const uint64_t k = lkeys[i];
    if (k == MZ_EMPTY) continue;
    MzRec r;
    r.cnt = lcnt[i];
    bool any = r.cnt != 0;
#pragma unroll
    for (int f = 0; f < MZ_SUMS; ++f) {
      r.s[f] = lsum[i * MZ_SUMS + f];
      any |= r.s[f] != 0;
    }
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      r.lo[f] = lbox[i * 6 + f];
      r.hi[f] = lbox[i * 6 + 3 + f];
    }
    if (any) mz_global_add(t, k, r, negate);
  }
}

// a cell is a key, a count, MZ_SUMS x u64 of sums and 6 x u32 of box; finalize gives the moments and the faces as two columns
struct MeasureCells {
  typedef MzTable Table;
  struct Out {
    uint64_t* keys;
    uint64_t* counts;
    uint32_t* box;
    uint64_t* sums;
    uint64_t* faces;
  };
  static constexpr size_t SLOT_BYTES = 16 + 8 * MZ_SUMS + 24;
  static constexpr int HEADER_CELLS = 0;
  static void layout(MzTable& t, int64_t capacity) {
    t.sums = t.counts + capacity;
    t.box = (uint32_t*)(t.sums + capacity * MZ_SUMS);
  }
  static __device__ void clear(const MzTable& t, int64_t i) {
    for (int f = 0; f < MZ_SUMS; ++f) t.sums[i * MZ_SUMS + f] = 0;
    for (int f = 0; f < 3; ++f) {
      t.box[i * 6 + f] = 0xffffffffu;
      t.box[i * 6 + 3 + f] = 0u;
    }
  }
  static __device__ void move(const MzTable& from, int64_t i, uint64_t k, uint64_t w, const MzTable& to) {
    MzRec r;
    r.cnt = w;
    for (int f = 0; f < MZ_SUMS; ++f) r.s[f] = from.sums[i * MZ_SUMS + f];
    for (int f = 0; f < 3; ++f) {
      r.lo[f] = from.box[i * 6 + f];
      r.hi[f] = from.box[i * 6 + 3 + f];
    }
    mz_global_add(to, k, r, 0);
  }
  static __device__ void write(const MzTable& t, int64_t i, const Out& out, int64_t pos) {
    for (int f = 0; f < 6; ++f) out.box[pos * 6 + f] = t.box[i * 6 + f];
    for (int f = 0; f < MZ_FACES; ++f) out.sums[pos * MZ_FACES + f] = t.sums[i * MZ_SUMS + f];
    for (int f = 0; f < 3; ++f) out.faces[pos * 3 + f] = t.sums[i * MZ_SUMS + MZ_FACES + f];
  }
};

struct MzSlab {
  const void* a;
  const void* halo;
  int64_t n, z0, D;
  int H, W, per_slice, border;
};

template <int S>
int mz_launch(const MzSlab& g, int is_signed, const MzTable& t, int negate, hipStream_t s) {
  constexpr int64_t TILE = (int64_t)MZ_THREADS * (16 / S);
  const int64_t ntiles = (g.n + TILE - 1) / TILE;
  const int64_t per = (ntiles + MZ_MAX_GRID - 1) / MZ_MAX_GRID;
  const int grid = (int)((ntiles + per - 1) / per);
  hipLaunchKernelGGL((label_measure_kernel<S>), dim3(grid), dim3(MZ_THREADS), 0, s, g.a, g.halo, g.n, is_signed, per, t, (uint32_t)g.H,
                     (uint32_t)g.W, (uint32_t)g.z0, (uint32_t)g.D, 1.0f / (float)g.H, 1.0f / (float)g.W, g.per_slice, g.border, negate);
  EMP_LAUNCH_CHECK();
  return EMP_OK;
}

int mz_dispatch(const MzSlab& g, int in_bytes, const MzTable& t, int negate, hipStream_t s) {
  const int sg = in_bytes < 0, A = sg ? -in_bytes : in_bytes;
  if (A == 1) return mz_launch<1>(g, sg, t, negate, s);
  if (A == 2) return mz_launch<2>(g, sg, t, negate, s);
  if (A == 4) return mz_launch<4>(g, sg, t, negate, s);
  if (A == 8) return mz_launch<8>(g, sg, t, negate, s);
  set_error("label_measure: element size %d unsupported (1, 2, 4, 8; negative = signed)", in_bytes);
  return EMP_ERR_INVALID;
}

}  // namespace
}  // namespace emp

using namespace emp;

extern "C" {

size_t emp_label_measure_work_bytes(int64_t capacity) {
  return cells_capacity_ok(capacity) ? CELL_HEADER + (size_t)capacity * MeasureCells::SLOT_BYTES : 0;
}

int emp_label_measure_reset(void* d_table, int64_t capacity, void* stream) {
  EMP_REQUIRE(d_table && cells_capacity_ok(capacity), "label_measure_reset: the capacity must be a power of two in [64, 2^32]");
  return cells_reset<MeasureCells>(d_table, capacity, (hipStream_t)stream);
}

// Synchronises the stream (it reads the table's flags).  *h_overflow = 1: the table was too small for this slab; what the call
// had added has been taken out again.
int emp_label_measure_accumulate(const void* d_labels, int in_bytes, int64_t z0, int depth, int H, int W, int64_t total_depth,
                                 const void* d_halo, int per_slice, int border_faces, void* d_table, int64_t capacity, void* stream,
                                 int* h_overflow) {
  EMP_REQUIRE(d_table && cells_capacity_ok(capacity) && h_overflow && depth >= 0 && H > 0 && W > 0 && (depth == 0 || d_labels),
              "label_measure_accumulate: bad arguments");
  EMP_REQUIRE(z0 >= 0 && total_depth >= z0 + depth, "label_measure_accumulate: the slab [%lld, %lld) does not lie in a volume of depth %lld",
              (long long)z0, (long long)(z0 + depth), (long long)total_depth);
  const int64_t big = total_depth > H ? (total_depth > W ? total_depth : W) : (H > W ? H : W);
  EMP_REQUIRE((unsigned __int128)big * big * total_depth * H * W < ((unsigned __int128)1 << 63),
              "label_measure_accumulate: a raw second moment could wrap: max(D, H, W)^2 * D * H * W must stay below 2^63, got shape (%lld, %d, %d)",
              (long long)total_depth, H, W);
  per_slice = per_slice != 0;
  EMP_REQUIRE(per_slice || z0 == 0 || depth == 0 || d_halo, "label_measure_accumulate: a slab that starts at slice %lld needs the slice below it (d_halo)",
              (long long)z0);
  hipStream_t s = (hipStream_t)stream;
  *h_overflow = 0;
  MzSlab g;
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
  const MzTable t = cells_table<MeasureCells>(d_table, capacity);
  return cells_accumulate(t.hdr, s, "label_measure_accumulate", "the key's domain (negative, or beyond 2^63 / per slice 2^32)",
                          [&](int negate) { return mz_dispatch(g, in_bytes, t, negate, s); }, h_overflow);
}

// Moves the cells of a table into an empty (reset) larger one.  Synchronises; *h_overflow = 1: d_to is too small as well.
int emp_label_measure_grow(const void* d_from, int64_t from_capacity, void* d_to, int64_t to_capacity, void* stream, int* h_overflow) {
  EMP_REQUIRE(d_from && d_to && cells_capacity_ok(from_capacity) && cells_capacity_ok(to_capacity) && to_capacity > from_capacity && h_overflow,
              "label_measure_grow: bad arguments");
  return cells_grow<MeasureCells>(d_from, from_capacity, d_to, to_capacity, (hipStream_t)stream, h_overflow);
}

// Synchronises.  *h_num = number of keys; the first min(*h_num, max_out) of them are written.
int emp_label_measure_finalize(void* d_table, int64_t capacity, uint64_t* d_keys, uint64_t* d_counts, uint32_t* d_boxes, uint64_t* d_sums,
                               uint64_t* d_faces, int64_t max_out, int64_t* h_num, void* stream) {
  EMP_REQUIRE(d_table && cells_capacity_ok(capacity) && h_num && max_out >= 0 && (max_out == 0 || (d_keys && d_counts && d_boxes && d_sums && d_faces)),
              "label_measure_finalize: bad arguments");
  return cells_finalize<MeasureCells>(d_table, capacity, {d_keys, d_counts, d_boxes, d_sums, d_faces}, max_out, h_num, (hipStream_t)stream);
}

}  // extern "C"
