// Morph Labels on the device (empanada_napari/_merge_split_widget.py:46-209): binary dilation, erosion, closing and opening
// of single labels of a label image / volume with a disk or ball of radius 1..7, each label within its own padded box.
//   per label (:123-134):  box of the label as the array is now, padded by the radius and clipped to the array (:56-67);
//                          binary = crop == label; crop[binary] = 0; binary = op(binary, footprint); crop[binary] = label
//   footprints (:92-95):   skimage.morphology.disk(r) / ball(r): x^2 + y^2 (+ z^2) <= r^2 on a (2r + 1)-cube
//   the ops (:48-53):      Dilate, Erode, Close, Open (`Fill holes` is not built)
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
#include "common.h"

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

}  // extern "C"
