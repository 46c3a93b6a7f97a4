// Clean-up of label volumes on the device: the per-label table (voxel count and bounding box of every label that occurs)
// and the edit of a volume through a small `from -> to` map.  The two primitives behind the plugin's label tools:
//   emp_label_table_accumulate   regionprops_table(img, properties=('label', 'area')) of Filter Small Labels
//                                (empanada_napari/_filter_small_labels.py:16-23), the borders clear_border looks at (:45),
//                                regionprops(...).bbox of Jump to Label (_merge_split_widget.py:652-656) and np.unique of
//                                Count Labels / Find Next Available Label (_label_counter_widget.py:243, _merge_split_widget.py:730)
//   emp_label_apply_map          the `labels[labels == l] = v` pass per label of remove_label_from_image
//                                (_filter_small_labels.py:10-12,27-28), Delete Labels (_merge_split_widget.py:249-250) and
//                                Merge Labels (:385-387), all labels in one pass
// skimage is not available where this library is built: what regionprops_table / clear_border compute is restated from
// their documented behaviour (area = voxel count, bbox = min and exclusive max per axis, clear_border = the connected
// components that touch a face), not pinned against them.
//
// The table kernel follows overlap.hip's three stages: 16-byte loads and a wave-level merge of lanes whose voxels are all
// equal, a bounded-probe LDS table per workgroup over a contiguous stretch of tiles, one global update per occupied LDS
// slot and workgroup.  What differs: a run carries its geometry.  A run is an interval of the raveled slab; its box follows
// from its two ends: within one row it is [x0, x1]; over several rows of one slice the first row reaches the row's end and
// the last one starts at 0, so x is [0, W - 1] and y is [y0, y1]; over several slices the same holds for y.  In per-slice
// mode (key = slice << 32 | label) a run that crosses a slice end is split there.  The coordinates of a tile's first voxel
// are carried along the stretch, so that a run head costs a division (of an offset below W + 4096, by a float reciprocal and
// one correction) only where it leaves its row.
// LDS and global box fields are read before they are updated: a box converges after a few runs of its label, and from then
// on a run costs the probe, the 64-bit add and six LDS reads.
// Overflow: as in overlap.hip, slots are never released, so the same slab with negated weights takes out exactly the counts
// a failed call added.  The min / max updates of a failed call are not undone: they are idempotent and are the right values
// once the slab is counted again (cells whose count is 0 do not exist for grow / finalize).
// The table around the count kernel -- layout, reset, rehash, compaction, the host side of accumulate / grow / finalize -- is
// label_table.h's; LabelTableCells below tells it what a cell of this family is.
#include <vector>

#include "common.h"
#include "label_table.h"

namespace emp {
namespace {

constexpr int LT_THREADS = 256;
constexpr int LT_LDS_SLOTS = 512;        // 40 B per slot: 20 KiB of LDS per workgroup, 8 workgroups per CU
constexpr int LT_LDS_PROBES = 8;
constexpr int LT_GLOBAL_PROBES = 128;
constexpr int64_t LT_MAX_GRID = 8192;    // short stretches, as overlap.hip (finding 82)
constexpr uint64_t LT_EMPTY = CELL_EMPTY;      // keys lie in [0, 2^63)

typedef unsigned long long ull_t;

struct LtTable {
  uint64_t* hdr;
  uint64_t* keys;
  uint64_t* counts;
  uint32_t* box;
  uint64_t mask;
};

struct LtBox {
  uint32_t lo[3], hi[3];      // z, y, x
};

// w: the (possibly negated) weight; with_box 0: the count only (the negated pass)
__device__ __forceinline__ void lt_global_add(const LtTable& t, uint64_t key, uint64_t w, const LtBox& r, int with_box) {
  uint64_t s = ov_hash(key) & t.mask;
#pragma unroll 1
  for (int p = 0; p < LT_GLOBAL_PROBES; ++p) {
    uint64_t cur = __hip_atomic_load(&t.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == LT_EMPTY) {
      cur = atomicCAS((ull_t*)&t.keys[s], (ull_t)LT_EMPTY, (ull_t)key);
      if (cur == LT_EMPTY) cur = key;
    }
    if (cur == key) {
      atomicAdd((ull_t*)&t.counts[s], (ull_t)w);
      if (with_box) ov_box_update_global(&t.box[s * 6], r);
      return;
    }
    s = (s + 1) & t.mask;
  }
  atomicOr((unsigned int*)&t.hdr[1], 1u);      // dropped: the host undoes the slab and grows the table
}

struct LtCtx {
  uint64_t* lkeys;
  uint64_t* lcnt;
  uint32_t* lbox;
  LtTable t;
  uint32_t H, W, zoff;
  float invH, invW;
  int per_slice, negate;
};

__device__ __forceinline__ void lt_lds_add(const LtCtx& c, uint64_t key, uint64_t w, const LtBox& r) {
  uint32_t s = (uint32_t)ov_hash(key) & (LT_LDS_SLOTS - 1);
#pragma unroll 1
  for (int p = 0; p < LT_LDS_PROBES; ++p) {
    uint64_t cur = __hip_atomic_load(&c.lkeys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (cur == LT_EMPTY) {
      cur = atomicCAS((ull_t*)&c.lkeys[s], (ull_t)LT_EMPTY, (ull_t)key);
      if (cur == LT_EMPTY) cur = key;
    }
    if (cur == key) {
      atomicAdd((ull_t*)&c.lcnt[s], (ull_t)w);
      if (!c.negate) {
        // the six fields in three 8-byte reads; a field only moves one way, so a stale value costs a spare atomic at most
        uint32_t* b = &c.lbox[s * 6];
        uint32_t cur[6];
#pragma unroll
        for (int f = 0; f < 3; ++f) {
          const uint64_t two = __hip_atomic_load((uint64_t*)&b[2 * f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          cur[2 * f] = (uint32_t)two;
          cur[2 * f + 1] = (uint32_t)(two >> 32);
        }
#pragma unroll
        for (int f = 0; f < 3; ++f) {
          if (r.lo[f] < cur[f]) atomicMin(&b[f], r.lo[f]);
          if (r.hi[f] > cur[3 + f]) atomicMax(&b[3 + f], r.hi[f]);
        }
      }
      return;
    }
    s = (s + 1) & (LT_LDS_SLOTS - 1);
  }
  lt_global_add(c.t, key, c.negate ? 0ull - w : w, r, !c.negate);
}

// a run of len voxels of one label from offset o of the tile whose first voxel is (bz, by, bx): one entry, or one per slice
// in per-slice mode (at most len of them)
__device__ __forceinline__ void lt_run(const LtCtx& c, uint64_t label, uint32_t bx, uint32_t by, uint32_t bz, uint32_t o, uint32_t len) {
  uint32_t x0, y0, z0, x1, y1, z1;
  ov_coord(c, bx, by, bz, o, x0, y0, z0);
  ov_coord(c, bx, by, bz, o + len - 1, x1, y1, z1);
  for (uint32_t z = z0;; ++z) {
    const uint32_t ze = c.per_slice ? z : z1;      // the entry covers the slices z .. ze
    const bool first = z == z0, last = ze == z1, multi = ze != z;
    const uint32_t ys = first ? y0 : 0u, xs = first ? x0 : 0u, ye = last ? y1 : c.H - 1, xe = last ? x1 : c.W - 1;
    // rows ys .. ye of one slice: the first one from xs, the last one up to xe; several rows span the whole width, several
    // slices the whole height as well
    const uint64_t cnt = multi ? (uint64_t)len : (uint64_t)((int64_t)(ye - ys) * c.W + (int64_t)xe - (int64_t)xs + 1);
    const bool rows = multi || ys != ye;
    LtBox r;
    r.lo[0] = c.zoff + z;
    r.hi[0] = c.zoff + ze;
    r.lo[1] = multi ? 0u : ys;
    r.hi[1] = multi ? c.H - 1 : ye;
    r.lo[2] = rows ? 0u : xs;
    r.hi[2] = rows ? c.W - 1 : xe;
    lt_lds_add(c, c.per_slice ? ((uint64_t)(c.zoff + z) << 32) | label : label, cnt, r);
    if (last) break;
  }
}

// elements per lane and tile: LT_VECS 16-byte vectors, 16 elements at most (the run walk of a lane is unrolled).  In a uniform
// stretch a wave then has one run head per LT_VECS KiB, and the head's path -- coordinates, hash, probe, box -- is what the
// kernel spends its time in, not the loads (finding 83)
constexpr int LT_VECS = 2;
template <int S> struct LtLane { static constexpr int E = 16 * LT_VECS / S > 16 ? 16 : 16 * LT_VECS / S; };

template <int S>
__global__ void __launch_bounds__(LT_THREADS) label_table_kernel(const void* __restrict__ a, int64_t n, int is_signed, int vec_ok,
                                                                 int64_t tiles_per_wg, LtTable t, uint32_t H, uint32_t W, uint32_t zoff,
                                                                 float invH, float invW, int per_slice, int negate) {
  constexpr int E = LtLane<S>::E, EV = 16 / S;
  constexpr uint32_t TILE = LT_THREADS * E;
  __shared__ uint64_t lkeys[LT_LDS_SLOTS];
  __shared__ uint64_t lcnt[LT_LDS_SLOTS];
  __shared__ __attribute__((aligned(8))) uint32_t lbox[LT_LDS_SLOTS * 6];
  for (int i = threadIdx.x; i < LT_LDS_SLOTS; i += LT_THREADS) {
    lkeys[i] = LT_EMPTY;
    lcnt[i] = 0;
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      lbox[i * 6 + f] = 0xffffffffu;
      lbox[i * 6 + 3 + f] = 0u;
    }
  }
  __syncthreads();
  LtCtx c;
  c.lkeys = lkeys;
  c.lcnt = lcnt;
  c.lbox = lbox;
  c.t = t;
  c.H = H;
  c.W = W;
  c.zoff = zoff;
  c.invH = invH;
  c.invW = invW;
  c.per_slice = per_slice;
  c.negate = negate;
  const int lane = threadIdx.x & 63;
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
    uint64_t v[E];
#pragma unroll
    for (int h = 0; h < E / EV; ++h) {
      const int nh = nv - h * EV;
      ov_load<S, EV>(a, i0 + h * EV, nh >= EV ? EV : (nh > 0 ? nh : 0), vec_ok, v + h * EV);
    }
    bool uni = nv == E;
#pragma unroll
    for (int j = 0; j < E; ++j) {
      bad = bad || ov_key_out_of_range<S>(v[j], is_signed, per_slice);
      uni &= v[j] == v[0];
    }
    // a uniform lane continues the run of a uniform predecessor with the same label
    const uint64_t prev_v = (uint64_t)__shfl_up((ull_t)v[0], 1);
    const int prev_uni = __shfl_up((int)uni, 1);
    const bool head = !uni || lane == 0 || !prev_uni || prev_v != v[0];
    const uint64_t heads = __ballot(head);
    if (uni) {
      if (head) {
        const uint64_t above = lane == 63 ? 0ull : heads >> (lane + 1);
        const int lanes = above ? __ffsll((ull_t)above) : 64 - lane;      // up to the next head, or the end of the wave
        lt_run(c, v[0], bx, by, bz, o0, (uint32_t)lanes * E);
      }
    } else if (nv > 0) {
      uint64_t cur = v[0];
      uint32_t start = 0, len = 1;
#pragma unroll
      for (int j = 1; j < E; ++j) {
        if (j < nv) {
          if (v[j] == cur) {
            ++len;
          } else {
            lt_run(c, cur, bx, by, bz, o0 + start, len);
            cur = v[j];
            start = j;
            len = 1;
          }
        }
      }
      lt_run(c, cur, bx, by, bz, o0 + start, len);
    }
    ov_coord(c, bx, by, bz, TILE, bx, by, bz);
  }
  if (bad) atomicOr((unsigned int*)&t.hdr[1] + 1, 1u);
  __syncthreads();
  for (int i = threadIdx.x; i < LT_LDS_SLOTS; i += LT_THREADS) {
    const uint64_t k = lkeys[i], w = lcnt[i];
    if (k != LT_EMPTY && w != 0) {
      LtBox r;
#pragma unroll
      for (int f = 0; f < 3; ++f) {
        r.lo[f] = lbox[i * 6 + f];
        r.hi[f] = lbox[i * 6 + 3 + f];
      }
      lt_global_add(t, k, negate ? 0ull - w : w, r, !negate);
    }
  }
}

// a cell is a key, a count and 6 x u32 of box (min z, y, x, max z, y, x; inclusive)
struct LabelTableCells {
  typedef LtTable Table;
  struct Out {
    uint64_t* keys;
    uint64_t* counts;
    uint32_t* box;
  };
  static constexpr size_t SLOT_BYTES = 40;
  static constexpr int HEADER_CELLS = 0;
  static void layout(LtTable& t, int64_t capacity) { t.box = (uint32_t*)(t.counts + capacity); }
  static __device__ void clear(const LtTable& t, int64_t i) {
    for (int f = 0; f < 3; ++f) {
      t.box[i * 6 + f] = 0xffffffffu;
      t.box[i * 6 + 3 + f] = 0u;
    }
  }
  static __device__ void move(const LtTable& from, int64_t i, uint64_t k, uint64_t w, const LtTable& to) {
    LtBox r;
    for (int f = 0; f < 3; ++f) {
      r.lo[f] = from.box[i * 6 + f];
      r.hi[f] = from.box[i * 6 + 3 + f];
    }
    lt_global_add(to, k, w, r, 1);
  }
  static __device__ void write(const LtTable& t, int64_t i, const Out& out, int64_t pos) {
    for (int f = 0; f < 6; ++f) out.box[pos * 6 + f] = t.box[i * 6 + f];
  }
};

template <int S>
int lt_launch(const void* a, int64_t n, int is_signed, const LtTable& t, int64_t z0, int H, int W, int per_slice, int negate, hipStream_t s) {
  constexpr int E = LtLane<S>::E;
  const int64_t ntiles = (n + (int64_t)LT_THREADS * E - 1) / ((int64_t)LT_THREADS * E);
  const int64_t per = (ntiles + LT_MAX_GRID - 1) / LT_MAX_GRID;
  const int grid = (int)((ntiles + per - 1) / per);
  const int vec_ok = (uintptr_t)a % 16 == 0;
  hipLaunchKernelGGL((label_table_kernel<S>), dim3(grid), dim3(LT_THREADS), 0, s, a, n, is_signed, vec_ok, per, t, (uint32_t)H, (uint32_t)W,
                     (uint32_t)z0, 1.0f / (float)H, 1.0f / (float)W, per_slice, negate);
  EMP_LAUNCH_CHECK();
  return EMP_OK;
}

int lt_dispatch(const void* a, int in_bytes, int64_t n, const LtTable& t, int64_t z0, int H, int W, int per_slice, int negate, hipStream_t s) {
  const int sg = in_bytes < 0, A = sg ? -in_bytes : in_bytes;
  if (A == 1) return lt_launch<1>(a, n, sg, t, z0, H, W, per_slice, negate, s);
  if (A == 2) return lt_launch<2>(a, n, sg, t, z0, H, W, per_slice, negate, s);
  if (A == 4) return lt_launch<4>(a, n, sg, t, z0, H, W, per_slice, negate, s);
  if (A == 8) return lt_launch<8>(a, n, sg, t, z0, H, W, per_slice, negate, s);
  set_error("label_table: element size %d unsupported (1, 2, 4, 8; negative = signed)", in_bytes);
  return EMP_ERR_INVALID;
}

// ---------------------------------------------------------------------------
// the edit
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool lm_find(const uint64_t* __restrict__ mkeys, const uint64_t* __restrict__ mvals, uint64_t mask, uint64_t key,
                                        uint64_t& val) {
  uint64_t s = ov_hash(key) & mask;
  for (uint64_t p = 0; p <= mask; ++p) {      // emp_label_map_build leaves half of the slots empty: a miss ends at the first of them
    const uint64_t cur = mkeys[s];
    if (cur == key) {
      val = mvals[s];
      return true;
    }
    if (cur == LT_EMPTY) return false;
    s = (s + 1) & mask;
  }
  return false;
}

struct LaArgs {
  int64_t HW;
  uint64_t zoff;
  int per_slice, key_signed;
  const uint64_t* mkeys;
  const uint64_t* mvals;
  uint64_t mask;
};

// the E values sv of a lane (elements i0 .. i0 + nv) through the map, by their keys kv
template <int SK, int E>
__device__ __forceinline__ void la_edit(const LaArgs& g, const uint64_t* kv, uint64_t* sv, int64_t i0, int nv) {
  uint64_t any = 0;
#pragma unroll
  for (int j = 0; j < E; ++j) any |= kv[j];
  if (!any) return;      // background (key 0) is never looked up
  uint64_t z = 0;
  int64_t p = 0;
  if (g.per_slice) {
    z = (uint64_t)(i0 / g.HW);
    p = i0 - (int64_t)z * g.HW;
  }
  uint64_t last = LT_EMPTY, last_val = 0;
  bool last_found = false;
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const uint64_t k = kv[j];
    // a value outside the key's domain (the table entries raise on it) is in no map
    const bool skip = k == 0 || j >= nv ||
                      (SK == 8 ? (g.per_slice ? (k >> 32) != 0 : (k >> 63) != 0) : (g.key_signed && ((k >> (8 * SK - 1)) & 1)));
    if (!skip) {
      uint64_t full = k;
      if (g.per_slice) {
        const uint64_t zj = p + j < g.HW ? z : (uint64_t)((i0 + j) / g.HW);
        full = ((g.zoff + zj) << 32) | k;
      }
      if (full != last) {
        last = full;
        last_found = lm_find(g.mkeys, g.mvals, g.mask, full, last_val);
      }
      if (last_found) sv[j] = last_val;
    }
  }
}

// Several tiles of a stretch are loaded together: a lane has 16 bytes per tile and array, and one tile per wave in flight is
// too little to cover the memory latency of a pure stream (the table and overlap kernels read more per tile).  Four tiles of
// 4- and 8-byte labels, fewer of the narrow types, whose 8 or 16 elements per vector would cost the registers of the occupancy
constexpr int LA_LDS_SLOTS = 1024;      // maps of up to 512 entries: 16 KiB of LDS per workgroup
template <int E> struct LaBatch { static constexpr int N = E <= 4 ? 4 : (E == 8 ? 2 : 1); };

template <int SK, int SS>
__global__ void __launch_bounds__(256) label_apply_kernel(const void* key, const void* src, void* out, int64_t n, int vec_ok,
                                                          int64_t tiles_per_wg, LaArgs g) {
  constexpr int E = 16 / (SK > SS ? SK : SS);
  constexpr int64_t TILE = 256 * E;
  constexpr int LA_BATCH = LaBatch<E>::N;
  typedef typename OvVec<SK * E>::type KV;
  typedef typename OvVec<SS * E>::type SV;
  const int64_t ntiles = (n + TILE - 1) / TILE;
  const int64_t tile0 = (int64_t)blockIdx.x * tiles_per_wg;
  const int64_t tile1 = tile0 + tiles_per_wg < ntiles ? tile0 + tiles_per_wg : ntiles;
  const bool same = key == src;      // then SK == SS (the entry sees to it)
  // a small map (the usual one: a few hundred labels of a blob volume) is looked up in LDS: two dependent global loads per
  // lookup were what kept the first version of this kernel at 0.54 of the copy rate
  __shared__ uint64_t lmap[2 * LA_LDS_SLOTS];
  if (g.mask < (uint64_t)LA_LDS_SLOTS) {
    for (uint32_t i = threadIdx.x; i <= (uint32_t)g.mask; i += 256) {
      lmap[i] = g.mkeys[i];
      lmap[LA_LDS_SLOTS + i] = g.mvals[i];
    }
    __syncthreads();
    g.mkeys = lmap;
    g.mvals = lmap + LA_LDS_SLOTS;
  }
  for (int64_t tile = tile0; tile < tile1; tile += LA_BATCH) {
    const int64_t i0 = (tile * 256 + threadIdx.x) * E;
    if (vec_ok && tile + LA_BATCH <= tile1 && (tile + LA_BATCH) * TILE <= n) {      // whole tiles, aligned: vectors
      KV kraw[LA_BATCH];
      SV sraw[LA_BATCH];
#pragma unroll
      for (int u = 0; u < LA_BATCH; ++u) {
        kraw[u] = *(const KV*)((const typename OvElem<SK>::type*)key + i0 + u * TILE);
        if (!same) sraw[u] = *(const SV*)((const typename OvElem<SS>::type*)src + i0 + u * TILE);
      }
#pragma unroll
      for (int u = 0; u < LA_BATCH; ++u) {
        uint64_t kv[E], sv[E];
        ov_unpack<SK, E>(kraw[u], kv);
        if (same) {
#pragma unroll
          for (int j = 0; j < E; ++j) sv[j] = kv[j];
        } else {
          ov_unpack<SS, E>(sraw[u], sv);
        }
        la_edit<SK, E>(g, kv, sv, i0 + u * TILE, E);
        *(SV*)((typename OvElem<SS>::type*)out + i0 + u * TILE) = ov_pack<SS, E>(sv);
      }
    } else {
      for (int u = 0; u < LA_BATCH && tile + u < tile1; ++u) {
        const int64_t iu = i0 + u * TILE;
        const int64_t left = n - iu;
        const int nv = left >= E ? E : (left > 0 ? (int)left : 0);
        if (nv == 0) continue;
        uint64_t kv[E], sv[E];
        ov_load<SK, E>(key, iu, nv, vec_ok, kv);
        if (same) {
#pragma unroll
          for (int j = 0; j < E; ++j) sv[j] = kv[j];
        } else {
          ov_load<SS, E>(src, iu, nv, vec_ok, sv);
        }
        la_edit<SK, E>(g, kv, sv, iu, nv);
        ov_store<SS, E>(out, iu, nv, vec_ok, sv);
      }
    }
  }
}

template <int SK, int SS>
int la_launch(const void* key, int key_signed, const void* src, void* out, int64_t n, int64_t HW, int64_t z0, int per_slice,
              const uint64_t* mkeys, const uint64_t* mvals, int64_t cap, hipStream_t s) {
  constexpr int E = 16 / (SK > SS ? SK : SS);
  const int64_t ntiles = (n + 256ll * E - 1) / (256ll * E);
  const int64_t per = (ntiles + LT_MAX_GRID - 1) / LT_MAX_GRID;
  const int grid = (int)((ntiles + per - 1) / per);
  const int vec_ok = (uintptr_t)key % (SK * E) == 0 && (uintptr_t)src % (SS * E) == 0 && (uintptr_t)out % (SS * E) == 0;
  LaArgs g;
  g.HW = HW;
  g.zoff = (uint64_t)z0;
  g.per_slice = per_slice;
  g.key_signed = key_signed;
  g.mkeys = mkeys;
  g.mvals = mvals;
  g.mask = (uint64_t)cap - 1;
  hipLaunchKernelGGL((label_apply_kernel<SK, SS>), dim3(grid), dim3(256), 0, s, key, src, out, n, vec_ok, per, g);
  EMP_LAUNCH_CHECK();
  return EMP_OK;
}

}  // namespace
}  // namespace emp

using namespace emp;

extern "C" {

size_t emp_label_table_work_bytes(int64_t capacity) {
  return cells_capacity_ok(capacity) ? CELL_HEADER + (size_t)capacity * LabelTableCells::SLOT_BYTES : 0;
}

int emp_label_table_reset(void* d_table, int64_t capacity, void* stream) {
  EMP_REQUIRE(d_table && cells_capacity_ok(capacity), "label_table_reset: the capacity must be a power of two in [64, 2^32]");
  return cells_reset<LabelTableCells>(d_table, capacity, (hipStream_t)stream);
}

// Synchronises the stream (it reads the table's flags).  *h_overflow = 1: the table was too small for this slab; the counts
// the call had added have been taken out again.
int emp_label_table_accumulate(const void* d_labels, int in_bytes, int64_t z0, int depth, int H, int W, int per_slice, void* d_table,
                               int64_t capacity, void* stream, int* h_overflow) {
  EMP_REQUIRE(d_table && cells_capacity_ok(capacity) && h_overflow && depth >= 0 && H > 0 && W > 0 && (depth == 0 || d_labels),
              "label_table_accumulate: bad arguments");
  EMP_REQUIRE(z0 >= 0 && z0 + depth <= 0x7fffffffll && W < 0x7fffffff - 8192 && H < 0x7fffffff - 8192,
              "label_table_accumulate: slice index, height or width beyond 2^31 - 2^13");
  hipStream_t s = (hipStream_t)stream;
  *h_overflow = 0;
  const int64_t n = (int64_t)depth * H * W;
  if (n == 0) return EMP_OK;
  const LtTable t = cells_table<LabelTableCells>(d_table, capacity);
  per_slice = per_slice != 0;
  return cells_accumulate(t.hdr, s, "label_table_accumulate", "the key's domain (negative, or beyond 2^63 / per slice 2^32)",
                          [&](int negate) { return lt_dispatch(d_labels, in_bytes, n, t, z0, H, W, per_slice, negate, s); }, h_overflow);
}

// Moves the cells of a table into an empty (reset) larger one.  Synchronises; *h_overflow = 1: d_to is too small as well.
int emp_label_table_grow(const void* d_from, int64_t from_capacity, void* d_to, int64_t to_capacity, void* stream, int* h_overflow) {
  EMP_REQUIRE(d_from && d_to && cells_capacity_ok(from_capacity) && cells_capacity_ok(to_capacity) && to_capacity > from_capacity && h_overflow,
              "label_table_grow: bad arguments");
  return cells_grow<LabelTableCells>(d_from, from_capacity, d_to, to_capacity, (hipStream_t)stream, h_overflow);
}

// Synchronises.  *h_num = number of keys; the first min(*h_num, max_out) of them are written.
int emp_label_table_finalize(void* d_table, int64_t capacity, uint64_t* d_keys, uint64_t* d_counts, uint32_t* d_boxes, int64_t max_out,
                             int64_t* h_num, void* stream) {
  EMP_REQUIRE(d_table && cells_capacity_ok(capacity) && h_num && max_out >= 0 && (max_out == 0 || (d_keys && d_counts && d_boxes)),
              "label_table_finalize: bad arguments");
  return cells_finalize<LabelTableCells>(d_table, capacity, {d_keys, d_counts, d_boxes}, max_out, h_num, (hipStream_t)stream);
}

// The map is built on the host (linear probing, the kernels' hash) and copied: n entries are a few megabytes at most.
// Synchronises (the staging vectors live on this call's stack).
int emp_label_map_build(const uint64_t* h_keys, const uint64_t* h_vals, int64_t n, uint64_t* d_map_keys, uint64_t* d_map_vals,
                        int64_t map_capacity, void* stream) {
  EMP_REQUIRE(n >= 0 && (n == 0 || (h_keys && h_vals)) && d_map_keys && d_map_vals && cells_capacity_ok(map_capacity) && map_capacity >= 2 * n,
              "label_map_build: the capacity must be a power of two in [64, 2^32], at least twice the number of entries");
  std::vector<uint64_t> keys((size_t)map_capacity, LT_EMPTY), vals((size_t)map_capacity, 0);
  const uint64_t mask = (uint64_t)map_capacity - 1;
  for (int64_t i = 0; i < n; ++i) {
    EMP_REQUIRE((h_keys[i] >> 63) == 0, "label_map_build: key %lld outside [0, 2^63)", (long long)i);
    uint64_t s = ov_hash(h_keys[i]) & mask;
    while (keys[s] != LT_EMPTY && keys[s] != h_keys[i]) s = (s + 1) & mask;      // ends: half of the slots stay empty
    keys[s] = h_keys[i];
    vals[s] = h_vals[i];      // a key given twice keeps its last value
  }
  hipStream_t s = (hipStream_t)stream;
  EMP_CHECK_HIP(hipMemcpyAsync(d_map_keys, keys.data(), keys.size() * 8, hipMemcpyHostToDevice, s));
  EMP_CHECK_HIP(hipMemcpyAsync(d_map_vals, vals.data(), vals.size() * 8, hipMemcpyHostToDevice, s));
  EMP_CHECK_HIP(hipStreamSynchronize(s));
  return EMP_OK;
}

int emp_label_apply_map(const void* d_key, int key_bytes, const void* d_src, int src_bytes, void* d_out, int64_t z0, int depth, int H, int W,
                        int per_slice, const uint64_t* d_map_keys, const uint64_t* d_map_vals, int64_t map_capacity, void* stream) {
  EMP_REQUIRE(depth >= 0 && H > 0 && W > 0 && z0 >= 0 && z0 + depth <= 0x7fffffffll && d_map_keys && d_map_vals && cells_capacity_ok(map_capacity),
              "label_apply_map: bad arguments");
  const int64_t n = (int64_t)depth * H * W;
  if (n == 0) return EMP_OK;
  EMP_REQUIRE(d_key && d_src && d_out, "label_apply_map: null array");
  const int ks = key_bytes < 0, K = ks ? -key_bytes : key_bytes, S = src_bytes < 0 ? -src_bytes : src_bytes;
  EMP_REQUIRE(d_key != d_src || K == S, "label_apply_map: one array with two element sizes");
  hipStream_t s = (hipStream_t)stream;
  const int64_t HW = (int64_t)H * W;
  per_slice = per_slice != 0;
#define LA_CASE(X, Y) \
  if (K == X && S == Y) return la_launch<X, Y>(d_key, ks, d_src, d_out, n, HW, z0, per_slice, d_map_keys, d_map_vals, map_capacity, s);
  LA_CASE(1, 1) LA_CASE(1, 2) LA_CASE(1, 4) LA_CASE(1, 8)
  LA_CASE(2, 1) LA_CASE(2, 2) LA_CASE(2, 4) LA_CASE(2, 8)
  LA_CASE(4, 1) LA_CASE(4, 2) LA_CASE(4, 4) LA_CASE(4, 8)
  LA_CASE(8, 1) LA_CASE(8, 2) LA_CASE(8, 4) LA_CASE(8, 8)
#undef LA_CASE
  set_error("label_apply_map: element sizes %d / %d unsupported (1, 2, 4, 8; negative = signed)", key_bytes, src_bytes);
  return EMP_ERR_INVALID;
}

}  // extern "C"
