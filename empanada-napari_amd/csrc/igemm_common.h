// What the MFMA implicit-GEMM convolution kernels that stage both operands by LDS-DMA share: conv_igemm.hip (128 x 128 family,
// also compiled as the grouped kernel), conv_igemm256.hip (256 x 256, its whole-line form and the half tile), conv_igemm_s64.hip
// (deep-ring 64 x 64), conv3x3c64.hip (register weights), conv16x3p.hip (fp16x3 over hl32 maps) and, for the activation and the
// barrier, conv16x3.hip and sepconv_common.h.  They are one design cut several times: an XCD-aware tile raster, pixel rows
// decoded once into (iy0, ix0, image), a K walk [group of kg slabs][tap][slab] with one bounds test per tap and a zero page for
// what falls outside, 1 KiB LDS-DMA pieces with the swizzle on the source address.  Everything here is independent of a
// kernel's tile shape and schedule; which piece is issued in which MFMA's shadow, every counted s_waitcnt, the sched_barrier /
// setprio placement, the prologues, tails and epilogues stay in the kernels.
//
// The rule for what lives here (FINDINGS 95, 96): an always-inline callee is simplified on its own before it is inlined, so a
// helper can reorder a whole kernel.  A kernel uses a helper only where every instantiation stayed the instruction stream it
// was.  That is why the K-walk counter, the fragment offsets, the accumulator clear, the MFMA block and the bias fetch are
// still written out in the kernels, and why conv_igemm_s64, the 128 x 128 family and conv16x3p keep their own pixel-row decode.
//
// Internal linkage throughout: the translation units land in one shared library.
#pragma once
#include "common.h"

namespace emp {

namespace {

// LDS row (x within a 32-cout group) -> cout within the group: x = t*16 + i (t = cout-tile parity, i = MFMA row) ->
// (i>>2)*8 + t*4 + (i&3).  Two cout tiles are interleaved at staging time so that a lane owns 8 consecutive couts.
__device__ __forceinline__ int perm32(int x) {
  const int t = x >> 4, i = x & 15;
  return ((i >> 2) << 3) + (t << 2) + (i & 3);
}

// epilogue activation: 0 none | 1 ReLU | 2 SiLU (x * sigmoid(x), bifpn.py:35,91).  Compile-time ACT: a run-time switch inside the
// unrolled epilogue costs ~6 scalar branches PER ELEMENT [measured: 470-850 s_cbranch per kernel, the epilogue of a 256 x 256
// tile took ~10 us]
template <int ACT>
__device__ __forceinline__ float conv_act(float x) {
  if (ACT == 1) return fmaxf(x, 0.f);
  if (ACT == 2) return x / (1.f + __expf(-x));
  return x;
}

__device__ __forceinline__ void lds_barrier() {
  // Raw barrier that orders LDS traffic only.  A fence (or __syncthreads) would also drain vmcnt: an in-flight
  // LDS-DMA is a pending LDS write on the VM counter.  The "memory" clobber keeps the compiler from moving
  // memory accesses across it; DMA completion is handled by the counted vmcnt waits of the issuing waves.
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// one LDS-DMA instruction: every lane's 16 bytes at `src` to dst + lane * 16 (dst wave-uniform: 1 KiB per wave)
__device__ __forceinline__ void lds_dma16(const void* src, void* dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}

// 64-byte LDS rows (a 32-channel K-tile): 16-byte chunk c of row r lives at chunk c ^ ((-(r >> 2)) & 3), conflict-free for the
// ds_read_b128 lane groups of gfx950; the swizzle is applied to the DMA source address, the destination is lane-linear.
// stage_chunk64: the logical chunk that lane l of a 16-row piece (row l >> 2) fetches.
__device__ __forceinline__ int stage_chunk64(int l) { return (l & 3) ^ ((-(l >> 4)) & 3); }

// XCD-aware raster: workgroup bid runs on XCD bid & 7; the 8 XCDs get contiguous ranges of pixel tiles (neighbouring tiles
// share input rows through the XCD's L2) and the cout tiles of one pixel tile run back to back on the same XCD.  ngroup > 0 is
// the intermediate raster (round 6): the XCD keeps `ngroup` cout tiles resident and walks ALL its pixel
// tiles under them, then the next group -- the weights (ngroup x K x 512 B) survive the rounds' output in L2, the activations
// are re-read nt / ngroup times instead of the weights mt_per_xcd times.  False: the workgroup has no tile.
__device__ __forceinline__ bool tile_of_block(int bid, int mt, int nt, int mt_per_xcd, int ngroup, int& mtile, int& ntile) {
  const int xcd = bid & 7, j = bid >> 3;
  mtile = xcd * mt_per_xcd + j / nt;
  ntile = j % nt;
  if (ngroup > 0) {
    const int per = mt_per_xcd * ngroup, g = j / per, rem = j - g * per;
    mtile = xcd * mt_per_xcd + rem / ngroup;
    ntile = g * ngroup + rem % ngroup;
  }
  return mtile < mt;
}

// ---- pixel rows: output pixel m = (n, oy, ox) decoded once ----
// Rows past M and taps outside the image read the zero page with a zero increment (iy0 = ix0 = -(1 << 28) fails every bounds
// test), so the staging loops are branch-free.  `chunk` is the lane's offset into the row in halfs, `ks` the halfs a K step
// advances.  Pointer form: the image base (+ chunk) of the row's pixel, the pointwise shortcut (1x1 / stride 1 / no padding:
// the source is the row itself) and the row's pixel in the second source (ConvParams::in2) at stride2.
template <typename P>
__device__ __forceinline__ const half_t* second_source_row(const P& p, int m, int HoWo, int chunk) {
  const int n = m / HoWo;
  const int r = m - n * HoWo;
  const int oy = r / p.Wo;
  const int ox = r - oy * p.Wo;
  return p.in2 + (((size_t)n * p.H2 + oy * p.stride2) * p.W2 + ox * p.stride2) * p.in2_ld + chunk;
}
template <typename P>
__device__ __forceinline__ void pixel_row_ptr(const P& p, int m, int HoWo, bool pointwise, int chunk, int ks, const half_t*& img, int& iy0,
                                              int& ix0, const half_t*& cur, int& inc, const half_t*& two) {
  img = p.in;
  iy0 = ix0 = -(1 << 28);
  cur = p.zero;
  inc = 0;
  two = p.zero;
  if (m < p.M) {
    if (p.in2) two = second_source_row(p, m, HoWo, chunk);
    if (pointwise) {
      cur = p.in + (size_t)m * p.in_ld + chunk;
      inc = ks;
    } else {
      const int n = m / HoWo;
      const int r = m - n * HoWo;
      const int oy = r / p.Wo;
      const int ox = r - oy * p.Wo;
      iy0 = oy * p.stride - p.pad;
      ix0 = ox * p.stride - p.pad;
      img = p.in + (size_t)n * p.H * p.W * p.in_ld + chunk;
    }
  }
}
// 32-bit pixel-index form (maps of fewer than 2^31 pixels): pix = the image's first pixel; row_halfs = halfs per pixel row
template <typename P>
__device__ __forceinline__ void pixel_row_pix(const P& p, int m, int HoWo, bool pointwise, int row_halfs, int first, int ks, int& iy0, int& ix0,
                                              int& pix, const half_t*& cur, int& inc) {
  iy0 = ix0 = -(1 << 28);
  pix = 0;
  cur = p.zero;
  inc = 0;
  if (m < p.M) {
    if (pointwise) {
      cur = p.in + (size_t)m * row_halfs + first;
      inc = ks;
    } else {
      const int n = m / HoWo;
      const int r = m - n * HoWo;
      const int oy = r / p.Wo;
      const int ox = r - oy * p.Wo;
      iy0 = oy * p.stride - p.pad;
      ix0 = ox * p.stride - p.pad;
      pix = n * p.H * p.W;
    }
  }
}

// ---- the tap test of the K walk [group of kg slabs][tap][slab], once per tap and group: tap (dy, dx) of a row -> its source at
// channel offset c0, or the zero page with a zero increment ----
__device__ __forceinline__ void tap_src(const half_t* img, int iy0, int ix0, int dy, int dx, int H, int W, int in_ld, int c0, const half_t* zero,
                                        int ks, const half_t*& cur, int& inc) {
  const int iy = iy0 + dy, ix = ix0 + dx;
  const bool ok = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
  cur = ok ? img + ((size_t)iy * W + ix) * in_ld + c0 : zero;
  inc = ok ? ks : 0;
}
__device__ __forceinline__ void tap_src_pix(const half_t* in, int pix, int iy0, int ix0, int dy, int dx, int H, int W, int row_halfs, int c0,
                                            const half_t* zero, int ks, const half_t*& cur, int& inc) {
  const int iy = iy0 + dy, ix = ix0 + dx;
  const bool ok = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
  cur = ok ? in + ((size_t)(pix + iy * W + ix) * row_halfs + c0) : zero;
  inc = ok ? ks : 0;
}

// ---- host side ----
// K-walk group in slabs per tap: kg == 0 -> 8 slabs (256 channels of the 32-channel kernels); a 1x1 convolution, a group larger
// than the tap or one that does not divide it walk tap-major (one group)
inline int default_kgroup(int KT, int CB, int kg, int dflt = 8) {
  if (kg == 0) kg = dflt;
  if (KT == 1 || kg > CB || CB % kg != 0) kg = CB;
  return kg;
}
// mt / nt / mt_per_xcd of a BM x BN tiling -> the grid of tile_of_block's raster
template <typename P>
inline int fill_raster(P& p, int BM, int BN) {
  p.mt = cdiv(p.M, BM);
  p.nt = cdiv(p.Cout, BN);
  p.mt_per_xcd = cdiv(p.mt, 8);
  return 8 * p.mt_per_xcd * p.nt;
}
// an A/B switch of the environment that is on only when set to the character c (env_on / env_int: common.h)
inline bool env_is(const char* name, char c) {
  const char* e = getenv(name);
  return e && e[0] == c;
}
// launch with dynamic LDS above the 64 KiB default
template <typename K, typename P>
inline int launch_dyn(K kernel, int grid, int block, int lds_bytes, hipStream_t stream, const P& p) {
  if (int rc = ensure_dyn_lds(reinterpret_cast<const void*>(kernel), lds_bytes)) return rc;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds_bytes, stream, p);
  EMP_LAUNCH_CHECK();
  return EMP_OK;
}

}  // namespace

}  // namespace emp
