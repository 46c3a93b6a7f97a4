// What the three fused separable-conv kernels share: sepconv.hip (fp16), sepconv_precise.hip (fp16 maps, fp32 taps, hi + lo
// depthwise result) and sepconv_x3.hip (fp32 maps).  They are one design -- a persistent workgroup per CU, "dw" waves that
// produce the B tiles of an 8 x 16-pixel output tile chunk by chunk, "mma" waves that multiply the previous step's tiles, one
// LDS-only barrier per step -- cut three times for three arithmetics.  Everything here is independent of the arithmetic: the
// tile geometry, the parameter block, the small device helpers, the two halves of the head epilogue and the host side of a
// launch.  The depthwise and MFMA roles themselves, the channel-chunk width (64 fp16 / 32 fp32 channels: 128 B per pixel
// either way) and the B-tile layouts stay with the kernels.
//
// Internal linkage throughout: the three translation units land in one shared library.
#pragma once
#include <type_traits>

#include "igemm_common.h"

namespace emp {

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int SC_TH = 8, SC_TW = 16;                  // output tile (rows x cols) = 128 pixels
// halo tile of a KS x KS depthwise kernel: (8 + KS - 1) rows x 20 columns of 128-byte pixels (KS = 5: 12 x 20 = 240 pixels =
// 30 LDS-DMA instructions of 8 pixels; KS = 3: 10 x 20 = 200 pixels = 25 instructions, the two right-most columns unused)
constexpr int SC_IW = SC_TW + 4;
constexpr int sc_npix(int ks) { return (SC_TH + ks - 1) * SC_IW; }
constexpr int sc_halo_bytes(int ks) { return sc_npix(ks) * 128; }
constexpr int SC_NDW = 4, SC_NMW = 4;                 // depthwise / mma waves where a kernel fixes them (one of each per SIMD)
constexpr int SC_MAX_LDS = 160 * 1024;

// T: element type of the maps (and of the zero page they are padded from), TW: element type of the depthwise taps.
// `act` is read by the host side only (the kernels take it as a template argument).
template <typename T, typename TW>
struct SepParams {
  const T* in;
  int N, H, W, C, in_ld;
  const TW* dww;         // depthwise taps, in the order the family's kernel reads them
  const half_t* pww;     // pointwise weights in the family's MFMA-fragment order
  const float* bias;     // [Cout]
  T* out;                // (N,H,W,out_ld) or nullptr (head mode)
  int out_ld, act;
  const T* zero;         // >= 2 KiB of zeros
  int tiles_x, tiles_y;
  int tiles;
  const float* hw;       // head mode: [hc][Cout] fp32
  const float* hb;       // [hc]
  int hc;
  float* hout;           // (N,hc) planes of `plane` floats
  int64_t plane;
};

__device__ __forceinline__ void tile_coords(int tiles_x, int tiles_y, int tile, int& n, int& y0, int& x0) {
  const int tx = tile % tiles_x;
  const int r = tile / tiles_x;
  const int ty = r % tiles_y;
  n = r / tiles_y;
  y0 = ty * SC_TH;
  x0 = tx * SC_TW;
}

// fp32 pair -> fp16 hi pair + fp16 lo pair: hi = rtz(x), lo = rtz(x - hi) (the residual is exact in fp32; v_cvt_pkrtz
// converts two values per instruction, the residual is one v_fma_mix / v_sub per value).  hi + lo is short of x by less than
// 2^-21 2^floor(log2 |x|) for |x| >= 2^-3 (22 bits) and by less than 2^-24 below (lo subnormal); from 65520 on hi is +-65504,
// not inf, and lo carries the rest up to a total of 131008 (measured on gfx950, FINDINGS 102)
__device__ __forceinline__ void split_hi_lo(const f32x2& x, f16x2& hi, f16x2& lo) {
  typedef __fp16 h2 __attribute__((ext_vector_type(2)));
  const h2 h = __builtin_amdgcn_cvt_pkrtz(x[0], x[1]);
  const h2 l = __builtin_amdgcn_cvt_pkrtz(x[0] - (float)h[0], x[1] - (float)h[1]);
  hi = __builtin_bit_cast(f16x2, h);
  lo = __builtin_bit_cast(f16x2, l);
}

// ---- head epilogue of an mma wave.  Its accumulators: tile t, pixel row nt, element e <-> cout wm*16*MT + (t>>1)*32 + g16*8 +
// (t&1)*4 + e at pixel (nt, n16) of the 8 x 16 tile.  What the lanes' indices enter is computed by the kernels and handed
// in (hp0, fy, fx): inside a kernel the compiler folds that arithmetic into lane arithmetic it already has, and a helper that
// derives it again from wm / g16 / fpx changes the instructions of code far from the call (FINDINGS 95).

// head, first half, one plane: sum[nt] = this lane's share of head_w[h] . y at pixel row nt, y being the activated accumulators;
// hp0 = the lane's weights of plane h, hwl + h*COUT + wm*16*MT + g16*8.  The fmaf order fixes the bits.
template <int MT>
__device__ __forceinline__ void head_plane_sums(const f32x4 (&acc)[MT][8], const float* hp0, float (&sum)[8]) {
#pragma unroll
  for (int nt = 0; nt < 8; ++nt) sum[nt] = 0.f;
#pragma unroll
  for (int blk = 0; blk < MT / 2; ++blk) {
    const float* hp = hp0 + blk * 32;
    float hv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) hv[e] = hp[e];
#pragma unroll
    for (int nt = 0; nt < 8; ++nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sum[nt] = fmaf(acc[2 * blk][nt][e], hv[e], sum[nt]);
        sum[nt] = fmaf(acc[2 * blk + 1][nt][e], hv[4 + e], sum[nt]);
      }
  }
}

// head, second half, a step later: the finishing lane of plane fh and pixel fpx = (fy, fx) of the tile adds the NMW waves'
// shares (red[wave][pixel][2]) to the head bias fhb and stores one float of plane fh
template <int NMW, class P>
__device__ __forceinline__ void head_store(const P p, const float* red, int tile, int fh, int fpx, int fy, int fx, float fhb) {
  int n, y0, x0;
  tile_coords(p.tiles_x, p.tiles_y, tile, n, y0, x0);
  const int oy = y0 + fy, ox = x0 + fx;
  float v = fhb;
#pragma unroll
  for (int wv = 0; wv < NMW; ++wv) v += red[(wv * 128 + fpx) * 2 + fh];
  if (oy < p.H && ox < p.W) p.hout[((size_t)n * p.hc + fh) * p.plane + (size_t)oy * p.W + ox] = v;
}

// ---- host side

// the halo ring, the two B tiles of bt_bytes and, for a head, its weights and the nmw waves' partial sums
constexpr size_t sep_lds_bytes(int ks, int bt_bytes, int Cout, int head_c, int nmw) {
  return 3 * sc_halo_bytes(ks) + 2 * bt_bytes + (head_c ? (size_t)2 * Cout * 4 + (size_t)nmw * 128 * 2 * 4 : 0);
}

inline bool sep_couts_supported(int Cout, int head_c) { return (Cout == 128 || Cout == 256) && head_c >= 0 && head_c <= 2; }

// one workgroup per CU, a multiple of 8 (the kernels deal tiles to the 8 XCDs)
inline int persistent_grid(int& grid) {
  static int n_cu = 0;
  if (!n_cu) {
    int dev = 0;
    EMP_CHECK_HIP(hipGetDevice(&dev));
    EMP_CHECK_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    n_cu = n_cu >= 8 ? (n_cu / 8) * 8 : 8;
  }
  grid = n_cu;
  return EMP_OK;
}

// The checks every family makes after its own shape rule, in their order, and the fields they share.  `fam` prefixes the
// messages; `aligned` is the family's own 16-byte rule.  dww, pww, bias and zero stay with the caller.
template <class P, typename T>
int sep_fill_params(P& p, const char* fam, const T* in, int N, int H, int W, int C, int in_ld, int act, T* out, int out_ld,
                    bool aligned, const float* head_w, const float* head_b, int head_c, float* hout, int64_t plane) {
  EMP_REQUIRE(act >= 0 && act <= 2, "%s: bad activation %d", fam, act);
  EMP_REQUIRE((head_c > 0) != (out != nullptr), "%s: exactly one of the feature / head outputs", fam);
  EMP_REQUIRE(aligned, "%s: 16-byte row alignment", fam);
  p.in = in; p.N = N; p.H = H; p.W = W; p.C = C; p.in_ld = in_ld;
  p.out = out; p.out_ld = out_ld; p.act = act;
  p.tiles_x = cdiv(W, SC_TW); p.tiles_y = cdiv(H, SC_TH);
  const int64_t tiles = (int64_t)N * p.tiles_x * p.tiles_y;
  EMP_REQUIRE(tiles < (1ll << 30), "%s: too many tiles", fam);
  p.tiles = (int)tiles;
  p.hw = head_w; p.hb = head_b; p.hc = head_c; p.hout = hout; p.plane = plane;
  return EMP_OK;
}

// Launches the ACT = p.act instantiation of a kernel on the persistent grid.  kern(std::integral_constant<int, ACT>) returns
// the instantiation's address.
template <class K, class P>
int launch_by_act(K kern, const P& p, int threads, size_t lds_bytes, hipStream_t s) {
  int grid = 0;
  if (int rc = persistent_grid(grid)) return rc;
  auto go = [&](auto k) -> int {
    if (int rc = ensure_dyn_lds(reinterpret_cast<const void*>(k), SC_MAX_LDS)) return rc;
    hipLaunchKernelGGL(k, dim3(grid), dim3(threads), lds_bytes, s, p);
    EMP_LAUNCH_CHECK();
    return EMP_OK;
  };
  if (p.act == 1) return go(kern(std::integral_constant<int, 1>{}));
  if (p.act == 2) return go(kern(std::integral_constant<int, 2>{}));
  return go(kern(std::integral_constant<int, 0>{}));
}

}  // namespace

}  // namespace emp
