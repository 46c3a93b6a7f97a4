// Scoring of label volumes: the exact sparse contingency table of two label arrays on the device, and the instance
// matching that the reference's two scoring paths derive from it.
//
// Device (gfx950):
//   emp_label_overlap_accumulate   for every pair (a[i], b[i]) that occurs, the uint64 number of voxels -- what
//                                  np.histogram2d(gt.ravel(), pred.ravel(), bins over the label VALUES) holds in its non-zero
//                                  cells (empanada_napari/_accuracy_metrics.py:123-131) and what rle_iou computes pair by pair
//                                  (empanada/inference/matcher.py:199-204), without a matrix over label values
//   emp_label_overlap_finalize     the occupied cells as (key = a << 32 | b, count), unsorted
// Host (C++):
//   emp_overlap_match              areas, IoU and the assignment (_accuracy_metrics.py:129-146, matcher.py:194-224)
//
// The count kernel is a pure stream over both arrays.  Three stages keep atomics away from the voxel rate
// (one global atomic per voxel would put every workgroup on the row of the (0, 0) pair):
//   1. a lane loads E consecutive voxels of both arrays (16 bytes of the wider one); a lane whose E pairs are all equal
//      ("uniform") joins the run of its predecessor in the wave: only the first lane of a run of uniform lanes with one
//      pair counts it, weighted with the run length (one ballot; the idiom of sparse.hip's ccl_init_rows_kernel)
//   2. run heads are added to a per-workgroup LDS hash table (open addressing on the 64-bit pair, LDS atomics).  A
//      workgroup walks a CONTIGUOUS stretch of tiles, not a strided one: neighbouring tiles hold the same few labels,
//      so the 1 024 slots last for the whole stretch.  The stretches are short (up to 8 192 workgroups): the time of a
//      workgroup grows with the object boundaries in its stretch, and few long stretches left the chip waiting for the
//      slowest one (finding 82: 1 024 workgroups 0.45 of the copy rate per call, 8 192 workgroups 0.62)
//   3. every occupied LDS slot goes to the global table once per workgroup (64-bit compare-and-swap to claim a key,
//      64-bit add for the count)
// Every probe sequence is bounded: a full LDS neighbourhood sends the entry to the global table, a full global
// neighbourhood raises the overflow flag and drops the entry.  No loop waits on another lane, wave or workgroup.
// Slots are never released, so a key that was dropped once is dropped every time and a key that was stored once is found
// every time: running the same slab again with negated weights removes exactly what the failed call added.  That is how
// emp_label_overlap_accumulate leaves the table as it found it when it reports an overflow; the caller then moves the
// table to a larger one (emp_label_overlap_grow) and counts the slab again.
// This file has the count kernel, its probe loops and the argument checks of the entries.  The table around them -- layout,
// reset, rehash, compaction, and the host side of accumulate / grow / finalize -- is label_table.h's, which labels.hip and
// measure.hip use as well; OverlapCells below tells it what a cell of this family is.
#include <algorithm>
#include <vector>

#include "common.h"
#include "label_table.h"

namespace emp {
namespace {

constexpr int OV_THREADS = 256;
#ifndef OV_LDS_SLOTS
#define OV_LDS_SLOTS 1024                // 2 x 8 KiB of LDS per workgroup
#endif
constexpr int OV_LDS_PROBES = 8;
constexpr int OV_GLOBAL_PROBES = 128;
#ifndef OV_MAX_GRID
#define OV_MAX_GRID 8192                 // 32 workgroups per CU, 8 of them resident: short stretches even out the objects' share of work
#endif
constexpr uint64_t OV_EMPTY = CELL_EMPTY;      // the pair (2^32 - 1, 2^32 - 1) is legal: it is counted in hdr[0] instead

typedef unsigned long long ull_t;

struct OvTable {
  uint64_t* hdr;
  uint64_t* keys;
  uint64_t* counts;
  uint64_t mask;
};

__device__ __forceinline__ void ov_global_add(const OvTable& t, uint64_t key, uint64_t w) {
  if (key == OV_EMPTY) {
    atomicAdd((ull_t*)&t.hdr[0], (ull_t)w);
    return;
  }
  uint64_t s = ov_hash(key) & t.mask;
  for (int p = 0; p < OV_GLOBAL_PROBES; ++p) {
    uint64_t cur = __hip_atomic_load(&t.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == OV_EMPTY) {
      cur = atomicCAS((ull_t*)&t.keys[s], (ull_t)OV_EMPTY, (ull_t)key);
      if (cur == OV_EMPTY) cur = key;
    }
    if (cur == key) {
      atomicAdd((ull_t*)&t.counts[s], (ull_t)w);
      return;
    }
    s = (s + 1) & t.mask;
  }
  atomicOr((unsigned int*)&t.hdr[1], 1u);      // dropped: the host undoes the slab and grows the table
}

__device__ __forceinline__ void ov_lds_add(uint64_t* lkeys, uint64_t* lcnt, const OvTable& t, uint64_t key, uint64_t w, int negate) {
  if (key != OV_EMPTY) {
    uint32_t s = (uint32_t)ov_hash(key) & (OV_LDS_SLOTS - 1);
    for (int p = 0; p < OV_LDS_PROBES; ++p) {
      uint64_t cur = __hip_atomic_load(&lkeys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (cur == OV_EMPTY) {
        cur = atomicCAS((ull_t*)&lkeys[s], (ull_t)OV_EMPTY, (ull_t)key);
        if (cur == OV_EMPTY) cur = key;
      }
      if (cur == key) {
        atomicAdd((ull_t*)&lcnt[s], (ull_t)w);
        return;
      }
      s = (s + 1) & (OV_LDS_SLOTS - 1);
    }
  }
  ov_global_add(t, key, negate ? 0ull - w : w);
}

// values outside [0, 2^32): an 8-byte value with a high word (a negative int64 included), a signed narrower value with its sign bit
template <int S>
__device__ __forceinline__ bool ov_out_of_range(uint64_t v, int is_signed) {
  if (S == 8) return (v >> 32) != 0;
  return is_signed && ((v >> (8 * S - 1)) & 1);
}

// Diagnostic builds (-DOV_ABLATE=..., by hand; tools/overlap_bench.py times them through tools/with_lib.py; their tables are
// wrong on purpose): 1 = loads + run collapse only, the run heads go into a register; 2 = no flush of the LDS table.
// -DOV_LDS_SLOTS=... / -DOV_MAX_GRID=...: table size and workgroup count (finding 82 has what they measured).
#ifndef OV_ABLATE
#define OV_ABLATE 0
#endif
#if OV_ABLATE == 1
#define OV_ADD(k, w) (sink ^= (k) + (w))
#else
#define OV_ADD(k, w) ov_lds_add(lkeys, lcnt, t, (k), (w), negate)
#endif

template <int SA, int SB>
__global__ void __launch_bounds__(OV_THREADS) overlap_count_kernel(const void* __restrict__ a, const void* __restrict__ b, int64_t n,
                                                                   int signed_a, int signed_b, int vec_ok, int64_t tiles_per_wg,
                                                                   OvTable t, int negate) {
  constexpr int E = 16 / (SA > SB ? SA : SB);
  __shared__ uint64_t lkeys[OV_LDS_SLOTS];
  __shared__ uint64_t lcnt[OV_LDS_SLOTS];
  for (int i = threadIdx.x; i < OV_LDS_SLOTS; i += OV_THREADS) {
    lkeys[i] = OV_EMPTY;
    lcnt[i] = 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t ntiles = (n + (int64_t)OV_THREADS * E - 1) / ((int64_t)OV_THREADS * E);
  const int64_t tile0 = (int64_t)blockIdx.x * tiles_per_wg;
  const int64_t tile1 = tile0 + tiles_per_wg < ntiles ? tile0 + tiles_per_wg : ntiles;
  bool bad = false;
  uint64_t sink = 0;
  for (int64_t tile = tile0; tile < tile1; ++tile) {
    const int64_t i0 = (tile * OV_THREADS + threadIdx.x) * E;
    const int64_t left = n - i0;
    const int nv = left >= E ? E : (left > 0 ? (int)left : 0);
    uint64_t va[E], vb[E];
    ov_load<SA, E>(a, i0, nv, vec_ok, va);
    ov_load<SB, E>(b, i0, nv, vec_ok, vb);
    uint64_t key[E];
    bool uni = nv == E;
#pragma unroll
    for (int j = 0; j < E; ++j) {
      bad = bad || ov_out_of_range<SA>(va[j], signed_a) || ov_out_of_range<SB>(vb[j], signed_b);
      key[j] = (va[j] << 32) | (vb[j] & 0xffffffffull);
      uni &= key[j] == key[0];
    }
    // a uniform lane continues the run of a uniform predecessor with the same pair
    const uint64_t prev_key = (uint64_t)__shfl_up((ull_t)key[0], 1);
    const int prev_uni = __shfl_up((int)uni, 1);
    const bool head = !uni || lane == 0 || !prev_uni || prev_key != key[0];
    const uint64_t heads = __ballot(head);
    if (uni) {
      if (head) {
        const uint64_t above = lane == 63 ? 0ull : heads >> (lane + 1);
        const int lanes = above ? __ffsll((ull_t)above) : 64 - lane;      // up to the next head, or the end of the wave
        OV_ADD(key[0], (uint64_t)lanes * E);
      }
    } else if (nv > 0) {
      uint64_t cur = key[0], len = 1;
#pragma unroll
      for (int j = 1; j < E; ++j) {
        if (j < nv) {
          if (key[j] == cur) {
            ++len;
          } else {
            OV_ADD(cur, len);
            cur = key[j];
            len = 1;
          }
        }
      }
      OV_ADD(cur, len);
    }
  }
  if (OV_ABLATE == 1 && sink == 0x0123456789abcdefull) t.hdr[7] = sink;      // keeps the ablated loop alive; never true in practice
  if (bad) atomicOr((unsigned int*)&t.hdr[1] + 1, 1u);
  __syncthreads();
#if OV_ABLATE != 2
  for (int i = threadIdx.x; i < OV_LDS_SLOTS; i += OV_THREADS) {
    const uint64_t k = lkeys[i], c = lcnt[i];
    if (k != OV_EMPTY && c != 0) ov_global_add(t, k, negate ? 0ull - c : c);
  }
#endif
}
#undef OV_ADD

// a cell is a key and a count and nothing else; the pair that equals OV_EMPTY is the one cell in the header
struct OverlapCells {
  typedef OvTable Table;
  struct Out {
    uint64_t* keys;
    uint64_t* counts;
  };
  static constexpr size_t SLOT_BYTES = 16;
  static constexpr int HEADER_CELLS = 1;
  static void layout(OvTable&, int64_t) {}
  static __device__ void clear(const OvTable&, int64_t) {}
  static __device__ void move(const OvTable&, int64_t, uint64_t k, uint64_t c, const OvTable& to) { ov_global_add(to, k, c); }
  static __device__ void write(const OvTable&, int64_t, const Out&, int64_t) {}
};

template <int SA, int SB>
int ov_launch(const void* a, const void* b, int64_t n, int sa, int sb, const OvTable& t, int negate, hipStream_t s) {
  constexpr int E = 16 / (SA > SB ? SA : SB);
  const int64_t ntiles = (n + (int64_t)OV_THREADS * E - 1) / ((int64_t)OV_THREADS * E);
  const int64_t per = (ntiles + OV_MAX_GRID - 1) / OV_MAX_GRID;
  const int grid = (int)((ntiles + per - 1) / per);
  const int vec_ok = ((uintptr_t)a % (SA * E) == 0) && ((uintptr_t)b % (SB * E) == 0);
  hipLaunchKernelGGL((overlap_count_kernel<SA, SB>), dim3(grid), dim3(OV_THREADS), 0, s, a, b, n, sa, sb, vec_ok, per, t, negate);
  EMP_LAUNCH_CHECK();
  return EMP_OK;
}

int ov_dispatch(const void* a, int ab, const void* b, int bb, int64_t n, const OvTable& t, int negate, hipStream_t s) {
  const int sa = ab < 0, sb = bb < 0;
  const int A = sa ? -ab : ab, B = sb ? -bb : bb;
#define OV_CASE(X, Y) if (A == X && B == Y) return ov_launch<X, Y>(a, b, n, sa, sb, t, negate, s);
  OV_CASE(1, 1) OV_CASE(1, 2) OV_CASE(1, 4) OV_CASE(1, 8)
  OV_CASE(2, 1) OV_CASE(2, 2) OV_CASE(2, 4) OV_CASE(2, 8)
  OV_CASE(4, 1) OV_CASE(4, 2) OV_CASE(4, 4) OV_CASE(4, 8)
  OV_CASE(8, 1) OV_CASE(8, 2) OV_CASE(8, 4) OV_CASE(8, 8)
#undef OV_CASE
  set_error("label_overlap: element sizes %d / %d unsupported (1, 2, 4, 8; negative = signed)", ab, bb);
  return EMP_ERR_INVALID;
}

}  // namespace
}  // namespace emp

using namespace emp;

extern "C" {

size_t emp_label_overlap_work_bytes(int64_t capacity) {
  return cells_capacity_ok(capacity) ? CELL_HEADER + (size_t)capacity * OverlapCells::SLOT_BYTES : 0;
}

int emp_label_overlap_reset(void* d_table, int64_t capacity, void* stream) {
  EMP_REQUIRE(d_table && cells_capacity_ok(capacity), "label_overlap_reset: the capacity must be a power of two in [64, 2^32]");
  return cells_reset<OverlapCells>(d_table, capacity, (hipStream_t)stream);
}

// Synchronises the stream (it reads the table's flags).  *h_overflow = 1: the table was too small for this slab; what the
// call had added has been taken out again, the table is as before the call.
int emp_label_overlap_accumulate(const void* d_a, int a_bytes, const void* d_b, int b_bytes, int64_t n, void* d_table,
                                 int64_t capacity, void* stream, int* h_overflow) {
  EMP_REQUIRE(d_table && cells_capacity_ok(capacity) && n >= 0 && h_overflow && (n == 0 || (d_a && d_b)), "label_overlap_accumulate: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  *h_overflow = 0;
  if (n == 0) return EMP_OK;
  const OvTable t = cells_table<OverlapCells>(d_table, capacity);
  return cells_accumulate(t.hdr, s, "label_overlap_accumulate", "[0, 2^32) (negative, or too large for the 32-bit halves of a pair)",
                          [&](int negate) { return ov_dispatch(d_a, a_bytes, d_b, b_bytes, n, t, negate, s); }, h_overflow);
}

// Moves the cells of a table into an empty (reset) larger one.  Synchronises; *h_overflow = 1: d_to is too small as well
// (reset it, or a larger one, and call again: d_from is unchanged).
int emp_label_overlap_grow(const void* d_from, int64_t from_capacity, void* d_to, int64_t to_capacity, void* stream, int* h_overflow) {
  EMP_REQUIRE(d_from && d_to && cells_capacity_ok(from_capacity) && cells_capacity_ok(to_capacity) && to_capacity > from_capacity && h_overflow,
              "label_overlap_grow: bad arguments");
  return cells_grow<OverlapCells>(d_from, from_capacity, d_to, to_capacity, (hipStream_t)stream, h_overflow);
}

// Synchronises.  *h_num = number of distinct pairs; the first min(*h_num, max_out) of them are written.
int emp_label_overlap_finalize(void* d_table, int64_t capacity, uint64_t* d_keys, uint64_t* d_counts, int64_t max_out,
                               int64_t* h_num, void* stream) {
  EMP_REQUIRE(d_table && cells_capacity_ok(capacity) && h_num && max_out >= 0 && (max_out == 0 || (d_keys && d_counts)), "label_overlap_finalize: bad arguments");
  return cells_finalize<OverlapCells>(d_table, capacity, {d_keys, d_counts}, max_out, h_num, (hipStream_t)stream);
}

// HOST.  k cells (h_a[i], h_b[i]) -> h_count[i], sorted by (a, b), each pair once (emp_label_overlap_finalize's output after the sort).
// Labels: the non-zero values of each side in ascending order (np.unique) with their areas (all cells of the label, those against
// background included).  Matching: IoU = inter / (area_a + area_b - inter) in float64 for the cells with both labels non-zero,
// then linear_sum_assignment on that matrix, maximised, through the sparse solver.  index_space 0: rows / columns are the labels that
// occur (matcher.py:194-213); 1: a row / column for every integer 1..max label, as np.histogram2d's bins make it
// (_accuracy_metrics.py:123-146): the absent ones are empty, but they take part in the tie-breaking.  Out: the assigned pairs with
// a non-zero overlap, rows ascending, as indices into the label lists.  All output arrays hold k entries.
int emp_overlap_match(int64_t k, const int64_t* h_a, const int64_t* h_b, const int64_t* h_count, int index_space,
                      int64_t* h_a_labels, int64_t* h_a_areas, int64_t* n_a, int64_t* h_b_labels, int64_t* h_b_areas, int64_t* n_b,
                      int64_t* h_rows, int64_t* h_cols, double* h_iou, int64_t* h_inter, int64_t* n_match) {
  EMP_REQUIRE(k >= 0 && n_a && n_b && n_match && (index_space == 0 || index_space == 1), "overlap_match: bad arguments");
  EMP_REQUIRE(k == 0 || (h_a && h_b && h_count && h_a_labels && h_a_areas && h_b_labels && h_b_areas && h_rows && h_cols && h_iou && h_inter),
              "overlap_match: null argument");
  *n_a = *n_b = *n_match = 0;
  for (int64_t i = 0; i < k; ++i) {
    EMP_REQUIRE(h_a[i] >= 0 && h_b[i] >= 0 && h_count[i] > 0, "overlap_match: negative label or empty cell at %lld", (long long)i);
    EMP_REQUIRE(i == 0 || h_a[i] > h_a[i - 1] || (h_a[i] == h_a[i - 1] && h_b[i] > h_b[i - 1]), "overlap_match: cells not sorted by (a, b)");
  }
  // side a: the cells are grouped by a already
  std::vector<int64_t> row_of(k, -1);
  int64_t G = 0;
  for (int64_t i = 0; i < k; ++i) {
    if (h_a[i] == 0) continue;
    if (G == 0 || h_a_labels[G - 1] != h_a[i]) {
      h_a_labels[G] = h_a[i];
      h_a_areas[G] = 0;
      ++G;
    }
    h_a_areas[G - 1] += h_count[i];
    row_of[i] = G - 1;
  }
  // side b: sorted distinct values
  std::vector<int64_t> bl;
  bl.reserve(k);
  for (int64_t i = 0; i < k; ++i)
    if (h_b[i] != 0) bl.push_back(h_b[i]);
  std::sort(bl.begin(), bl.end());
  bl.erase(std::unique(bl.begin(), bl.end()), bl.end());
  const int64_t P = (int64_t)bl.size();
  for (int64_t j = 0; j < P; ++j) {
    h_b_labels[j] = bl[j];
    h_b_areas[j] = 0;
  }
  std::vector<int64_t> col_of(k, -1);
  for (int64_t i = 0; i < k; ++i) {
    if (h_b[i] == 0) continue;
    const int64_t j = std::lower_bound(bl.begin(), bl.end(), h_b[i]) - bl.begin();
    h_b_areas[j] += h_count[i];
    col_of[i] = j;
  }
  *n_a = G;
  *n_b = P;
  if (G == 0 || P == 0) return EMP_OK;
  std::vector<int64_t> er, ec, cell;
  std::vector<double> ew;
  for (int64_t i = 0; i < k; ++i) {
    if (row_of[i] < 0 || col_of[i] < 0) continue;
    const int64_t r = row_of[i], c = col_of[i];
    const double inter = (double)h_count[i];
    const double uni = (double)(h_a_areas[r] + h_b_areas[c]) - inter;
    er.push_back(index_space ? h_a[i] - 1 : r);
    ec.push_back(index_space ? h_b[i] - 1 : c);
    ew.push_back(inter / uni);
    cell.push_back(i);
  }
  const int64_t nr = index_space ? h_a_labels[G - 1] : G, nc = index_space ? h_b_labels[P - 1] : P;
  EMP_REQUIRE(nr <= (1ll << 26) && nc <= (1ll << 26), "overlap_match: labels beyond 2^26 in the per-value index space (use index_space 0)");
  const int64_t km = nr < nc ? nr : nc;
  std::vector<int64_t> rows(km), cols(km);
  const int rc = emp_lsa_maximize_sparse(nr, nc, (int64_t)er.size(), er.data(), ec.data(), ew.data(), rows.data(), cols.data());
  if (rc) return rc;
  // the assigned pairs that are cells: the entries are sorted by (row, column) like the cells they came from
  int64_t m = 0;
  for (int64_t q = 0; q < km; ++q) {
    size_t lo = 0, hi = er.size();
    while (lo < hi) {
      const size_t mid = (lo + hi) / 2;
      if (er[mid] < rows[q] || (er[mid] == rows[q] && ec[mid] < cols[q])) lo = mid + 1; else hi = mid;
    }
    if (lo == er.size() || er[lo] != rows[q] || ec[lo] != cols[q]) continue;
    const int64_t i = cell[lo];
    h_rows[m] = row_of[i];
    h_cols[m] = col_of[i];
    h_iou[m] = ew[lo];
    h_inter[m] = h_count[i];
    ++m;
  }
  *n_match = m;
  return EMP_OK;
}

}  // extern "C"
