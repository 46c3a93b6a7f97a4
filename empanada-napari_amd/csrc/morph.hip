// Morph Labels on the device (empanada_napari/_merge_split_widget.py:46-209): binary dilation, erosion, closing and opening
// of single labels of a label image / volume with a disk or ball of radius 1..7, each label within its own padded box.
//   per label (:123-134):  box of the label as the array is now, padded by the radius and clipped to the array (:56-67);
//                          binary = crop == label; crop[binary] = 0; binary = op(binary, footprint); crop[binary] = label
//   footprints (:92-95):   skimage.morphology.disk(r) / ball(r): x^2 + y^2 (+ z^2) <= r^2 on a (2r + 1)-cube
//   the ops (:48-53):      Dilate, Erode, Close, Open; `Fill holes` is the second half of this file
//   dilation:              scipy.ndimage.binary_dilation(structure=footprint): outside the crop is false
//   erosion:               scipy.ndimage.binary_erosion(structure=footprint, border_value=True): outside the CROP is true
//   Close = erode(dilate), Open = dilate(erode), each stage with its own rule for what lies outside the crop
// skimage is not available where this library is built: its binary_dilation / binary_erosion are restated from their
// documented behaviour (the two scipy calls above) and are not pinned against skimage itself.
//
// The host (labels.py, morph_schedule) orders the turns into levels: the turns of a level touch disjoint parts of the array,
// so a level is three launches over a list of tiles (turn, z, y, x) that covers the padded boxes of its turns:
//   morph_box_kernel    the box of every label of the level as the array is now (earlier levels may have eaten voxels);
//                       the first level takes its boxes from the label table and skips this launch
//   morph_mask_kernel   the new mask of a tile's core into a scratch buffer, nothing is written to the array
//   morph_apply_kernel  old voxels of the label -> 0, new mask -> label, within the crop
// The mask and the apply are two launches because neighbouring tiles of one label read each other's halo.
//
// A mask row is ONE 64-bit word: bit b of a tile's row is the voxel x0 - halo + b, halo = radius * stages (stages: 2 for Close
// and Open), and the tile's core is the 64 - 2 * halo bits in the middle.  A row is loaded by one wave with one ballot.  The
// footprint is, per (dz, dy), the row dilated along x by the half-width floor(sqrt(r^2 - dy^2 - dz^2)): log2 steps of
// d |= d << s | d >> s.  Bits that a shift drops or brings in at the ends of the word only reach the halo bits, whose results
// nobody reads: every stage shrinks the valid part of the word by the radius on both sides.
// Only dilation is computed: erosion by a symmetric footprint with `true` outside the crop is the complement of the dilation
// of the complement with `false` outside the crop.  So every stage is: (complement if erosion) -> clear outside the crop ->
// dilate -> (complement if erosion).
//
// Fill holes (:53, :90-91, emp_fill_holes_labels): binary = skimage.morphology.remove_small_holes(crop == label, hole_size), then
// crop[binary] = label.  The complement of the mask inside the CROP is split into its 4- / 6-connected components (connectivity
// 1, no diagonals) and every component with fewer than hole_size voxels (`<`) becomes the label, whatever it held and whether
// or not it touches the crop's border.  remove_small_holes / remove_small_objects are restated from their source and are not
// pinned against skimage either.  Same levels, same tile lists (a tile's row is 64 core voxels, there is no halo), and per
// level, after morph_box_kernel:
//   fill_init_kernel    a parent word and a size word per voxel of the level's frames -- a turn's frame is the host's padded and
//                       clipped box, which holds the crop; a voxel's entry is the frame's offset + its linear position in it, so
//                       the scratch is as large as the level's boxes, not as the array.  A background voxel of the crop starts
//                       under the first voxel of its horizontal run inside the wave, everything else is -1
//   fill_merge_kernel   lock-free union-find (union_find.h, shared with sparse.hip) with the x - 1, y - 1, z - 1 neighbours
//   fill_count_kernel   path compression, and one integer atomicAdd per run of a wave onto the root's size word
//   fill_apply_kernel   background voxels whose root's size is < hole_size get the label; nothing else is written
// All atomics are integer minima and sums: the result does not depend on their order.
#include "common.h"
#include "union_find.h"

namespace emp {
namespace {

constexpr int MP_THREADS = 256;
constexpr int MP_WAVES = MP_THREADS / 64;
constexpr int MP_MAX_R = 7;
constexpr int MP_MAX_FP = (2 * MP_MAX_R + 1) * (2 * MP_MAX_R + 1);
constexpr int MP_BALL_CZ = 8, MP_BALL_CY = 16, MP_DISK_CY = 64;
// rows of the loaded mask / of the intermediate one at radius 7, two stages: ball (8 + 28) * (16 + 28) and (8 + 14) * (16 + 14)
constexpr int MP_MAX_IN_ROWS = (MP_BALL_CZ + 4 * MP_MAX_R) * (MP_BALL_CY + 4 * MP_MAX_R);
constexpr int MP_MAX_MID_ROWS = (MP_BALL_CZ + 2 * MP_MAX_R) * (MP_BALL_CY + 2 * MP_MAX_R);
static_assert(MP_DISK_CY + 4 * MP_MAX_R <= MP_MAX_IN_ROWS && MP_DISK_CY + 2 * MP_MAX_R <= MP_MAX_MID_ROWS, "disk tile");
constexpr uint32_t MP_NO_BOX = 0xffffffffu;

struct MpGeom {
  int D, H, W;
  int r, ball, nst;
  int ero[2];         // stage s is an erosion
  int cz, cy, cx;     // a tile's core
  int halo, hz;       // halo along x and y; along z (0 for the disk)
};

inline bool mp_geom(int D, int H, int W, int radius, int ball, int op, MpGeom& g) {
  if (radius < 1 || radius > MP_MAX_R || op < 0 || op > 3 || D < 1 || H < 1 || W < 1 || (!ball && D != 1)) return false;
  g.D = D;
  g.H = H;
  g.W = W;
  g.r = radius;
  g.ball = ball != 0;
  g.nst = op >= 2 ? 2 : 1;
  g.ero[0] = op == EMP_MORPH_ERODE || op == EMP_MORPH_OPEN;
  g.ero[1] = op == EMP_MORPH_CLOSE;
  g.halo = radius * g.nst;
  g.hz = g.ball ? g.halo : 0;
  g.cz = g.ball ? MP_BALL_CZ : 1;
  g.cy = g.ball ? MP_BALL_CY : MP_DISK_CY;
  g.cx = 64 - 2 * g.halo;
  return true;
}

template <int S> struct MpElem;
template <> struct MpElem<1> { typedef uint8_t type; };
template <> struct MpElem<2> { typedef uint16_t type; };
template <> struct MpElem<4> { typedef uint32_t type; };
template <> struct MpElem<8> { typedef uint64_t type; };

struct MpBox {
  int lo[3], hi[3];      // z, y, x; inclusive
};

// the crop of a turn: its current box padded by the radius and clipped to the array; false: the label has no voxel left
__device__ __forceinline__ bool mp_crop(const MpGeom& g, const uint32_t* __restrict__ cur, MpBox& c) {
  if (cur[0] == MP_NO_BOX) return false;
  const int dim[3] = {g.D, g.H, g.W};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int pad = (a == 0 && !g.ball) ? 0 : g.r;
    const int lo = (int)cur[a] - pad, hi = (int)cur[3 + a] + pad;
    c.lo[a] = lo < 0 ? 0 : lo;
    c.hi[a] = hi > dim[a] - 1 ? dim[a] - 1 : hi;
  }
  return true;
}

__device__ __forceinline__ bool mp_core_meets_crop(const MpGeom& g, const MpBox& c, int z0, int y0, int x0) {
  return z0 <= c.hi[0] && z0 + g.cz > c.lo[0] && y0 <= c.hi[1] && y0 + g.cy > c.lo[1] && x0 <= c.hi[2] && x0 + g.cx > c.lo[2];
}

// the bits of the row (z, y) of a word whose bit 0 is the voxel xw0 that lie inside the crop
__device__ __forceinline__ uint64_t mp_crop_bits(const MpBox& c, int z, int y, int xw0) {
  if (z < c.lo[0] || z > c.hi[0] || y < c.lo[1] || y > c.hi[1]) return 0ull;
  const int lo = c.lo[2] - xw0 < 0 ? 0 : c.lo[2] - xw0;
  const int hi = c.hi[2] - xw0 > 63 ? 63 : c.hi[2] - xw0;
  if (lo > hi) return 0ull;
  return (~0ull >> (63 - hi)) & (~0ull << lo);
}

// w dilated along x by h: the reach doubles with every step (1, 3, 7), the last step is cut to what is left
__device__ __forceinline__ uint64_t mp_xdil(uint64_t w, int h) {
  uint64_t d = w;
  int done = 0, s = 1;
  while (done < h) {
    const int step = s < h - done ? s : h - done;
    d |= (d << step) | (d >> step);
    done += step;
    s <<= 1;
  }
  return d;
}

// ---------------------------------------------------------------------------
// the boxes of a level's labels as the array is now
// ---------------------------------------------------------------------------
template <int S>
__global__ void __launch_bounds__(MP_THREADS) morph_box_kernel(const void* __restrict__ vol, MpGeom g, const uint64_t* __restrict__ labels,
                                                               uint32_t* __restrict__ cur, const int32_t* __restrict__ tiles) {
  typedef typename MpElem<S>::type T;
  const int32_t* t = tiles + 4 * (int64_t)blockIdx.x;
  const int turn = t[0], z0 = t[1], y0 = t[2], x0 = t[3];
  const uint64_t label = labels[turn];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = x0 + lane - g.halo;
  const bool xin = lane >= g.halo && lane < 64 - g.halo && x < g.W;      // core bits only: the cores of a turn's tiles are disjoint
  uint32_t lo[3] = {MP_NO_BOX, MP_NO_BOX, MP_NO_BOX}, hi[3] = {0u, 0u, 0u};
  const int rows = g.cz * g.cy;
  for (int row = wave; row < rows; row += MP_WAVES) {
    const int z = z0 + row / g.cy, y = y0 + row % g.cy;
    bool p = false;
    if (xin && z < g.D && y < g.H) p = (uint64_t)((const T*)vol)[((int64_t)z * g.H + y) * g.W + x] == label;
    const uint64_t word = __ballot(p);
    if (word) {
      const uint32_t xl = (uint32_t)(x0 - g.halo + (__ffsll((unsigned long long)word) - 1));
      const uint32_t xh = (uint32_t)(x0 - g.halo + 63 - __clzll((long long)word));
      lo[0] = min(lo[0], (uint32_t)z);
      hi[0] = max(hi[0], (uint32_t)z);
      lo[1] = min(lo[1], (uint32_t)y);
      hi[1] = max(hi[1], (uint32_t)y);
      lo[2] = min(lo[2], xl);
      hi[2] = max(hi[2], xh);
    }
  }
  if (lane == 0 && lo[0] != MP_NO_BOX) {
    uint32_t* b = cur + 6 * (int64_t)turn;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMin(&b[a], lo[a]);
      atomicMax(&b[3 + a], hi[a]);
    }
  }
}

// ---------------------------------------------------------------------------
// the new mask of a tile's core
// ---------------------------------------------------------------------------
struct MpFootprint {
  int8_t dz[MP_MAX_FP], dy[MP_MAX_FP], h[MP_MAX_FP];
  int n;
};

// out (orz x ory rows) = the rows of in (rows iry long) dilated by the footprint; in has the radius as a halo around out
__device__ __forceinline__ uint64_t mp_dilate_row(const uint64_t* in, int iry, int oz, int oy, const MpGeom& g, const MpFootprint& fp) {
  const int bz = g.ball ? oz + g.r : oz, by = oy + g.r;
  uint64_t acc = 0;
  for (int k = 0; k < fp.n; ++k) {
    const uint64_t w = in[(bz + fp.dz[k]) * iry + by + fp.dy[k]];
    if (w) acc |= mp_xdil(w, fp.h[k]);
  }
  return acc;
}

template <int S>
__global__ void __launch_bounds__(MP_THREADS) morph_mask_kernel(const void* __restrict__ vol, MpGeom g, const uint64_t* __restrict__ labels,
                                                                const uint32_t* __restrict__ cur, const int32_t* __restrict__ tiles,
                                                                uint64_t* __restrict__ scratch) {
  typedef typename MpElem<S>::type T;
  __shared__ uint64_t in[MP_MAX_IN_ROWS];
  __shared__ uint64_t mid[MP_MAX_MID_ROWS];
  __shared__ MpFootprint fp;
  const int32_t* t = tiles + 4 * (int64_t)blockIdx.x;
  const int turn = t[0], z0 = t[1], y0 = t[2], x0 = t[3];
  MpBox c;
  if (!mp_crop(g, cur + 6 * (int64_t)turn, c) || !mp_core_meets_crop(g, c, z0, y0, x0)) return;      // uniform over the workgroup
  const uint64_t label = labels[turn];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int xw0 = x0 - g.halo;      // the voxel of bit 0

  if (threadIdx.x == 0) fp.n = 0;
  __syncthreads();
  const int side = 2 * g.r + 1;
  for (int i = threadIdx.x; i < side * side; i += MP_THREADS) {
    const int dz = i / side - g.r, dy = i % side - g.r;
    const int rem = g.r * g.r - dz * dz - dy * dy;
    if (rem < 0 || (!g.ball && dz != 0)) continue;
    int h = 0;
    while ((h + 1) * (h + 1) <= rem) ++h;
    const int k = atomicAdd(&fp.n, 1);      // the order of an OR does not matter
    fp.dz[k] = (int8_t)dz;
    fp.dy[k] = (int8_t)dy;
    fp.h[k] = (int8_t)h;
  }

  // the mask of `== label` over core + halo, four rows per wave and step so that their loads are in flight together
  const int irz = g.cz + 2 * g.hz, iry = g.cy + 2 * g.halo, irows = irz * iry;
  const int x = xw0 + lane;
  for (int base = wave * 4; base < irows; base += MP_WAVES * 4) {
    T v[4];
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = base + u;
      const int z = z0 - g.hz + row / iry, y = y0 - g.halo + row % iry;
      ok[u] = row < irows && z >= c.lo[0] && z <= c.hi[0] && y >= c.lo[1] && y <= c.hi[1] && x >= c.lo[2] && x <= c.hi[2];
      v[u] = 0;
      if (ok[u]) v[u] = ((const T*)vol)[((int64_t)z * g.H + y) * g.W + x];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = base + u;
      uint64_t word = __ballot(ok[u] && (uint64_t)v[u] == label);
      if (row < irows) {
        if (g.ero[0]) word = ~word & mp_crop_bits(c, z0 - g.hz + row / iry, y0 - g.halo + row % iry, xw0);
        if (lane == 0) in[row] = word;
      }
    }
  }
  __syncthreads();

  const int crows = g.cz * g.cy;
  uint64_t* out = scratch + (int64_t)blockIdx.x * crows;
  if (g.nst == 1) {
    for (int row = threadIdx.x; row < crows; row += MP_THREADS) {
      const uint64_t acc = mp_dilate_row(in, iry, row / g.cy, row % g.cy, g, fp);
      out[row] = g.ero[0] ? ~acc : acc;
    }
    return;
  }
  // two stages: the first one over the core and a halo of one radius, where it is cut to the crop for the second one
  const int mrz = g.cz + (g.ball ? 2 * g.r : 0), mry = g.cy + 2 * g.r, mrows = mrz * mry;
  for (int row = threadIdx.x; row < mrows; row += MP_THREADS) {
    const int oz = row / mry, oy = row % mry;
    uint64_t v = mp_dilate_row(in, iry, oz, oy, g, fp);
    if (g.ero[0] != g.ero[1]) v = ~v;      // the first stage's complement back, the second stage's complement in
    mid[row] = v & mp_crop_bits(c, z0 - (g.ball ? g.r : 0) + oz, y0 - g.r + oy, xw0);
  }
  __syncthreads();
  for (int row = threadIdx.x; row < crows; row += MP_THREADS) {
    const uint64_t acc = mp_dilate_row(mid, mry, row / g.cy, row % g.cy, g, fp);
    out[row] = g.ero[1] ? ~acc : acc;
  }
}

// ---------------------------------------------------------------------------
// the edit: crop[crop == label] = 0; crop[mask] = label
// ---------------------------------------------------------------------------
template <int S>
__global__ void __launch_bounds__(MP_THREADS) morph_apply_kernel(void* __restrict__ vol, MpGeom g, const uint64_t* __restrict__ labels,
                                                                 const uint32_t* __restrict__ cur, const int32_t* __restrict__ tiles,
                                                                 const uint64_t* __restrict__ scratch) {
  typedef typename MpElem<S>::type T;
  const int32_t* t = tiles + 4 * (int64_t)blockIdx.x;
  const int turn = t[0], z0 = t[1], y0 = t[2], x0 = t[3];
  MpBox c;
  if (!mp_crop(g, cur + 6 * (int64_t)turn, c) || !mp_core_meets_crop(g, c, z0, y0, x0)) return;      // the test of morph_mask_kernel
  const uint64_t label = labels[turn];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = x0 - g.halo + lane;
  const bool xin = lane >= g.halo && lane < 64 - g.halo && x >= c.lo[2] && x <= c.hi[2];
  const int crows = g.cz * g.cy;
  const uint64_t* mask = scratch + (int64_t)blockIdx.x * crows;
  for (int row = wave; row < crows; row += MP_WAVES) {
    const int z = z0 + row / g.cy, y = y0 + row % g.cy;
    if (!xin || z < c.lo[0] || z > c.hi[0] || y < c.lo[1] || y > c.hi[1]) continue;
    T* p = (T*)vol + ((int64_t)z * g.H + y) * g.W + x;
    const bool set = (mask[row] >> lane) & 1ull;
    const T old = *p;
    if (set) {
      if ((uint64_t)old != label) *p = (T)label;
    } else if ((uint64_t)old == label) {
      *p = (T)0;
    }
  }
}

template <int S>
int mp_run(void* vol, const MpGeom& g, const uint64_t* labels, uint32_t* cur, const int32_t* tiles, const int64_t* off, int n_levels,
           uint64_t* scratch, int64_t scratch_words, hipStream_t s, int* launches) {
  const int64_t crows = (int64_t)g.cz * g.cy;
  for (int l = 0; l < n_levels; ++l) {
    const int64_t n = off[l + 1] - off[l];
    EMP_REQUIRE(n >= 0 && n <= 0x7fffffffll && n * crows <= scratch_words, "morph_labels: level %d has %lld tiles, the scratch buffer holds %lld",
                l, (long long)n, (long long)(scratch_words / crows));
    if (n == 0) continue;
    const int32_t* lt = tiles + 4 * off[l];
    if (l > 0) {
      hipLaunchKernelGGL((morph_box_kernel<S>), dim3((unsigned)n), dim3(MP_THREADS), 0, s, (const void*)vol, g, labels, cur, lt);
      EMP_LAUNCH_CHECK();
      ++*launches;
    }
    hipLaunchKernelGGL((morph_mask_kernel<S>), dim3((unsigned)n), dim3(MP_THREADS), 0, s, (const void*)vol, g, labels, (const uint32_t*)cur, lt,
                       scratch);
    EMP_LAUNCH_CHECK();
    hipLaunchKernelGGL((morph_apply_kernel<S>), dim3((unsigned)n), dim3(MP_THREADS), 0, s, vol, g, labels, (const uint32_t*)cur, lt,
                       (const uint64_t*)scratch);
    EMP_LAUNCH_CHECK();
    *launches += 2;
  }
  return EMP_OK;
}

// ---------------------------------------------------------------------------
// Fill holes: the 4- / 6-connected components of `crop != label` of every turn of a level, their sizes, and the edit
// ---------------------------------------------------------------------------
struct FhScratch {
  const int64_t* frames;      // per turn {z0, y0, x0, nz, ny, nx, offset}
  int* parent;
  int* size;
  int64_t entries, n_turns;
};

struct FhTile {
  int z0, y0, x0;
  MpBox c;                    // the crop
  int f0[3], fn[3], off;      // the frame: first voxel, extent, first entry
  uint64_t label;
};

inline void fh_geom(int D, int H, int W, int radius, int ball, MpGeom& g) {
  g.D = D;
  g.H = H;
  g.W = W;
  g.r = radius;
  g.ball = ball != 0;
  g.nst = 1;
  g.ero[0] = g.ero[1] = 0;
  g.halo = g.hz = 0;      // no stencil: a tile's row is 64 core voxels
  g.cz = g.ball ? MP_BALL_CZ : 1;
  g.cy = g.ball ? MP_BALL_CY : MP_DISK_CY;
  g.cx = 64;
}

// The tile of this workgroup; false (uniform over the workgroup): nothing to do -- the label has no voxel left, or the core
// lies outside the crop: the test of morph_mask_kernel.  The crop lies inside the turn's frame (the host's box is where the
// label can be); it is cut to the frame all the same, and a frame that does not fit the scratch arrays is skipped, so that
// no index leaves them whatever the host passed.
__device__ __forceinline__ bool fh_tile(const MpGeom& g, const FhScratch& sc, const uint64_t* __restrict__ labels,
                                        const uint32_t* __restrict__ cur, const int32_t* __restrict__ tiles, FhTile& t) {
  const int32_t* q = tiles + 4 * (int64_t)blockIdx.x;
  const int turn = q[0];
  if (turn < 0 || turn >= sc.n_turns) return false;
  t.z0 = q[1];
  t.y0 = q[2];
  t.x0 = q[3];
  const int64_t* f = sc.frames + 7 * (int64_t)turn;
  const int dim[3] = {g.D, g.H, g.W};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (f[a] < 0 || f[3 + a] < 1 || f[a] + f[3 + a] > dim[a]) return false;
    t.f0[a] = (int)f[a];
    t.fn[a] = (int)f[3 + a];
  }
  if (f[6] < 0 || f[6] + f[3] * f[4] * f[5] > sc.entries) return false;
  t.off = (int)f[6];
  if (!mp_crop(g, cur + 6 * (int64_t)turn, t.c)) return false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    t.c.lo[a] = max(t.c.lo[a], t.f0[a]);
    t.c.hi[a] = min(t.c.hi[a], t.f0[a] + t.fn[a] - 1);
    if (t.c.lo[a] > t.c.hi[a]) return false;
  }
  if (!mp_core_meets_crop(g, t.c, t.z0, t.y0, t.x0)) return false;
  t.label = labels[turn];
  return true;
}

// the entry of the voxel (z, y, x) of the frame
__device__ __forceinline__ int fh_index(const FhTile& t, int z, int y, int x) {
  return t.off + ((z - t.f0[0]) * t.fn[1] + (y - t.f0[1])) * t.fn[2] + (x - t.f0[2]);
}

__device__ __forceinline__ bool fh_row_in_crop(const FhTile& t, int z, int y) {
  return z >= t.c.lo[0] && z <= t.c.hi[0] && y >= t.c.lo[1] && y <= t.c.hi[1];
}

template <int S>
__device__ __forceinline__ bool fh_background(const void* __restrict__ vol, const MpGeom& g, const FhTile& t, int z, int y, int x) {
  typedef typename MpElem<S>::type T;
  return (uint64_t)((const T*)vol)[((int64_t)z * g.H + y) * g.W + x] != t.label;
}

// A background voxel of the crop starts under the first voxel of its horizontal run inside the wave (one ballot, as
// sparse.hip's ccl_init_rows_kernel); every other voxel of the frame that the tile covers gets -1; all sizes start at 0.
template <int S>
__global__ void __launch_bounds__(MP_THREADS) fill_init_kernel(const void* __restrict__ vol, MpGeom g, const uint64_t* __restrict__ labels,
                                                               const uint32_t* __restrict__ cur, const int32_t* __restrict__ tiles,
                                                               FhScratch sc) {
  FhTile t;
  if (!fh_tile(g, sc, labels, cur, tiles, t)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = t.x0 + lane;
  const bool xf = x >= t.f0[2] && x < t.f0[2] + t.fn[2];
  const bool xc = x >= t.c.lo[2] && x <= t.c.hi[2];
  const int rows = g.cz * g.cy;
  for (int row = wave; row < rows; row += MP_WAVES) {
    const int z = t.z0 + row / g.cy, y = t.y0 + row % g.cy;
    if (z < t.f0[0] || z >= t.f0[0] + t.fn[0] || y < t.f0[1] || y >= t.f0[1] + t.fn[1]) continue;      // uniform over the wave
    const bool bg = xc && fh_row_in_crop(t, z, y) && fh_background<S>(vol, g, t, z, y, x);
    const uint64_t word = __ballot(bg);
    if (!xf) continue;
    const int idx = fh_index(t, z, y, x);
    int p = -1;
    if (bg) {
      const uint64_t stops = ~word & ((1ull << lane) - 1ull);      // the voxels before me that end a run
      p = idx - (lane - (stops ? 64 - __clzll((long long)stops) : 0));
    }
    sc.parent[idx] = p;
    sc.size[idx] = 0;
  }
}

// Unions with the x - 1, y - 1 and z - 1 neighbours, across tiles too, where they are not implied: a run inside the wave is
// joined already, and the union with the voxel above (or before, along z) is the left neighbour's when that one has the same
// two neighbours.
template <int S>
__global__ void __launch_bounds__(MP_THREADS) fill_merge_kernel(const void* __restrict__ vol, MpGeom g, const uint64_t* __restrict__ labels,
                                                                const uint32_t* __restrict__ cur, const int32_t* __restrict__ tiles,
                                                                FhScratch sc) {
  FhTile t;
  if (!fh_tile(g, sc, labels, cur, tiles, t)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = t.x0 + lane;
  const bool xc = x >= t.c.lo[2] && x <= t.c.hi[2];
  const int rows = g.cz * g.cy;
  for (int row = wave; row < rows; row += MP_WAVES) {
    const int z = t.z0 + row / g.cy, y = t.y0 + row % g.cy;
    if (!fh_row_in_crop(t, z, y)) continue;      // uniform over the wave
    const bool bg = xc && fh_background<S>(vol, g, t, z, y, x);
    const bool has_y = y > t.c.lo[1], has_z = z > t.c.lo[0];
    const uint64_t word = __ballot(bg);
    const uint64_t yword = __ballot(has_y && xc && fh_background<S>(vol, g, t, z, y - 1, x));
    const uint64_t zword = __ballot(has_z && xc && fh_background<S>(vol, g, t, z - 1, y, x));
    if (!bg) continue;
    const int idx = fh_index(t, z, y, x);
    const bool left = lane > 0 ? ((word >> (lane - 1)) & 1ull) != 0 : (x > t.c.lo[2] && fh_background<S>(vol, g, t, z, y, x - 1));
    if (lane == 0 && left) uf_union(sc.parent, idx, idx - 1);      // the run continues from the tile before
    const bool inside = lane > 0 && left;
    if (((yword >> lane) & 1ull) && !(inside && ((yword >> (lane - 1)) & 1ull))) uf_union(sc.parent, idx, idx - t.fn[2]);
    if (((zword >> lane) & 1ull) && !(inside && ((zword >> (lane - 1)) & 1ull))) uf_union(sc.parent, idx, idx - t.fn[1] * t.fn[2]);
  }
}

// Every background voxel under its root, and the length of every run inside a wave added to its root's size: one integer
// atomicAdd per run.
__global__ void __launch_bounds__(MP_THREADS) fill_count_kernel(MpGeom g, const uint64_t* __restrict__ labels, const uint32_t* __restrict__ cur,
                                                                const int32_t* __restrict__ tiles, FhScratch sc) {
  FhTile t;
  if (!fh_tile(g, sc, labels, cur, tiles, t)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = t.x0 + lane;
  const bool xc = x >= t.c.lo[2] && x <= t.c.hi[2];
  const int rows = g.cz * g.cy;
  for (int row = wave; row < rows; row += MP_WAVES) {
    const int z = t.z0 + row / g.cy, y = t.y0 + row % g.cy;
    if (!fh_row_in_crop(t, z, y)) continue;      // uniform over the wave
    int root = -1;
    if (xc) {
      const int idx = fh_index(t, z, y, x);
      const int p = uf_load(sc.parent, idx);
      if (p >= 0) {
        root = uf_find(sc.parent, p);
        if (root != p) sc.parent[idx] = root;
      }
    }
    const uint64_t word = __ballot(root >= 0);
    if (root >= 0 && (lane == 0 || !((word >> (lane - 1)) & 1ull))) {
      const uint64_t ends = ~(word >> lane);
      atomicAdd(&sc.size[root], ends ? __ffsll((unsigned long long)ends) - 1 : 64);
    }
  }
}

// crop[remove_small_holes(crop == label)] = label: the background voxels of components with fewer than hole_size voxels
template <int S>
__global__ void __launch_bounds__(MP_THREADS) fill_apply_kernel(void* __restrict__ vol, MpGeom g, const uint64_t* __restrict__ labels,
                                                                const uint32_t* __restrict__ cur, const int32_t* __restrict__ tiles,
                                                                FhScratch sc, int64_t hole_size) {
  typedef typename MpElem<S>::type T;
  FhTile t;
  if (!fh_tile(g, sc, labels, cur, tiles, t)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = t.x0 + lane;
  if (x < t.c.lo[2] || x > t.c.hi[2]) return;
  const int rows = g.cz * g.cy;
  for (int row = wave; row < rows; row += MP_WAVES) {
    const int z = t.z0 + row / g.cy, y = t.y0 + row % g.cy;
    if (!fh_row_in_crop(t, z, y)) continue;
    const int root = sc.parent[fh_index(t, z, y, x)];
    if (root >= 0 && (int64_t)sc.size[root] < hole_size) ((T*)vol)[((int64_t)z * g.H + y) * g.W + x] = (T)t.label;
  }
}

template <int S>
int fh_run(void* vol, const MpGeom& g, int64_t hole_size, const uint64_t* labels, uint32_t* cur, const int32_t* tiles, const int64_t* off,
           int n_levels, const FhScratch& sc, hipStream_t s, int* launches) {
  for (int l = 0; l < n_levels; ++l) {
    const int64_t n = off[l + 1] - off[l];
    EMP_REQUIRE(n >= 0 && n <= 0x7fffffffll, "fill_holes_labels: level %d has %lld tiles", l, (long long)n);
    if (n == 0) continue;
    const int32_t* lt = tiles + 4 * off[l];
    const dim3 grid((unsigned)n), block(MP_THREADS);
    if (l > 0) {
      hipLaunchKernelGGL((morph_box_kernel<S>), grid, block, 0, s, (const void*)vol, g, labels, cur, lt);
      EMP_LAUNCH_CHECK();
      ++*launches;
    }
    hipLaunchKernelGGL((fill_init_kernel<S>), grid, block, 0, s, (const void*)vol, g, labels, (const uint32_t*)cur, lt, sc);
    EMP_LAUNCH_CHECK();
    hipLaunchKernelGGL((fill_merge_kernel<S>), grid, block, 0, s, (const void*)vol, g, labels, (const uint32_t*)cur, lt, sc);
    EMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(fill_count_kernel, grid, block, 0, s, g, labels, (const uint32_t*)cur, lt, sc);
    EMP_LAUNCH_CHECK();
    hipLaunchKernelGGL((fill_apply_kernel<S>), grid, block, 0, s, vol, g, labels, (const uint32_t*)cur, lt, sc, hole_size);
    EMP_LAUNCH_CHECK();
    *launches += 4;
  }
  return EMP_OK;
}

}  // namespace
}  // namespace emp

using namespace emp;

extern "C" {

int emp_morph_tile_shape(int radius, int ball, int op, int* cz, int* cy, int* cx) {
  MpGeom g;
  EMP_REQUIRE(cz && cy && cx && mp_geom(1, 1, 1, radius, ball, op, g), "morph_tile_shape: radius 1..7, op 0..3");
  *cz = g.cz;
  *cy = g.cy;
  *cx = g.cx;
  return EMP_OK;
}

int emp_morph_labels(void* d_vol, int elem_bytes, int D, int H, int W, int radius, int ball, int op, const uint64_t* d_turn_labels,
                     uint32_t* d_turn_boxes, int64_t n_turns, const int32_t* d_tiles, const int64_t* h_level_offsets, int n_levels,
                     uint64_t* d_scratch, int64_t scratch_words, void* stream, int* h_launches) {
  MpGeom g;
  EMP_REQUIRE(mp_geom(D, H, W, radius, ball, op, g), "morph_labels: radius 1..7, op 0..3, a disk needs D == 1 (got radius %d, op %d, D %d)",
              radius, op, D);
  EMP_REQUIRE(n_levels >= 0 && n_turns >= 0 && h_level_offsets && h_launches, "morph_labels: bad arguments");
  *h_launches = 0;
  if (n_levels == 0 || h_level_offsets[n_levels] == 0) return EMP_OK;
  EMP_REQUIRE(d_vol && d_turn_labels && d_turn_boxes && d_tiles && d_scratch && h_level_offsets[0] == 0, "morph_labels: null array");
  hipStream_t s = (hipStream_t)stream;
  const int A = elem_bytes < 0 ? -elem_bytes : elem_bytes;
  if (A == 1) return mp_run<1>(d_vol, g, d_turn_labels, d_turn_boxes, d_tiles, h_level_offsets, n_levels, d_scratch, scratch_words, s, h_launches);
  if (A == 2) return mp_run<2>(d_vol, g, d_turn_labels, d_turn_boxes, d_tiles, h_level_offsets, n_levels, d_scratch, scratch_words, s, h_launches);
  if (A == 4) return mp_run<4>(d_vol, g, d_turn_labels, d_turn_boxes, d_tiles, h_level_offsets, n_levels, d_scratch, scratch_words, s, h_launches);
  if (A == 8) return mp_run<8>(d_vol, g, d_turn_labels, d_turn_boxes, d_tiles, h_level_offsets, n_levels, d_scratch, scratch_words, s, h_launches);
  set_error("morph_labels: element size %d unsupported (1, 2, 4, 8; negative = signed)", elem_bytes);
  return EMP_ERR_INVALID;
}

int emp_fill_holes_tile_shape(int ball, int* cz, int* cy, int* cx) {
  EMP_REQUIRE(cz && cy && cx, "fill_holes_tile_shape: null pointer");
  MpGeom g;
  fh_geom(1, 1, 1, 1, ball, g);
  *cz = g.cz;
  *cy = g.cy;
  *cx = g.cx;
  return EMP_OK;
}

int emp_fill_holes_labels(void* d_vol, int elem_bytes, int D, int H, int W, int radius, int ball, int64_t hole_size,
                          const uint64_t* d_turn_labels, uint32_t* d_turn_boxes, const int64_t* d_turn_frames, int64_t n_turns,
                          const int32_t* d_tiles, const int64_t* h_level_offsets, int n_levels, int32_t* d_parent, int32_t* d_size,
                          int64_t scratch_entries, void* stream, int* h_launches) {
  EMP_REQUIRE(radius >= 1 && radius <= MP_MAX_R && D >= 1 && H >= 1 && W >= 1 && (ball || D == 1),
              "fill_holes_labels: radius 1..7, without the ball D == 1 (got radius %d, D %d)", radius, D);
  EMP_REQUIRE(hole_size >= 0 && n_levels >= 0 && n_turns >= 0 && h_level_offsets && h_launches, "fill_holes_labels: bad arguments");
  EMP_REQUIRE(scratch_entries >= 0 && scratch_entries < 0x7fffffffll,
              "fill_holes_labels: the boxes of a level must hold fewer than 2^31 - 1 voxels (got %lld scratch entries)",
              (long long)scratch_entries);
  *h_launches = 0;
  if (hole_size <= 1 || n_levels == 0 || h_level_offsets[n_levels] == 0) return EMP_OK;      // no component has fewer than 1 voxel
  EMP_REQUIRE(d_vol && d_turn_labels && d_turn_boxes && d_turn_frames && d_tiles && d_parent && d_size && h_level_offsets[0] == 0,
              "fill_holes_labels: null array");
  MpGeom g;
  fh_geom(D, H, W, radius, ball, g);
  const FhScratch sc = {d_turn_frames, d_parent, d_size, scratch_entries, n_turns};
  hipStream_t s = (hipStream_t)stream;
  const int A = elem_bytes < 0 ? -elem_bytes : elem_bytes;
  if (A == 1) return fh_run<1>(d_vol, g, hole_size, d_turn_labels, d_turn_boxes, d_tiles, h_level_offsets, n_levels, sc, s, h_launches);
  if (A == 2) return fh_run<2>(d_vol, g, hole_size, d_turn_labels, d_turn_boxes, d_tiles, h_level_offsets, n_levels, sc, s, h_launches);
  if (A == 4) return fh_run<4>(d_vol, g, hole_size, d_turn_labels, d_turn_boxes, d_tiles, h_level_offsets, n_levels, sc, s, h_launches);
  if (A == 8) return fh_run<8>(d_vol, g, hole_size, d_turn_labels, d_turn_boxes, d_tiles, h_level_offsets, n_levels, sc, s, h_launches);
  set_error("fill_holes_labels: element size %d unsupported (1, 2, 4, 8; negative = signed)", elem_bytes);
  return EMP_ERR_INVALID;
}

}  // extern "C"
