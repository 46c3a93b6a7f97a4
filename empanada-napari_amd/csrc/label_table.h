// The growable open-addressing table in which the label tools keep one cell per key on the device (overlap.hip: pair counts;
// labels.hip: count + box; measure.hip: count + box + 12 sums): everything about it that does not depend on what a cell holds.
//
// Layout: a 64-byte header -- hdr[1] = flags (u32 overflow, u32 range), hdr[2] = compaction cursor, hdr[0] a family's own --
// then `capacity` keys, `capacity` counts, and whatever else a family keeps per slot.  A key of CELL_EMPTY marks a free slot.
// Slots are never released, and a cell whose count is 0 does not exist (it was claimed by a slab that has been undone).
//
// A family describes its cells in a struct F:
//   Table         what its kernels take: hdr, keys, counts, mask, and pointers to the rest of a slot
//   Out           the output arrays of finalize: keys, counts, and one pointer per further column
//   SLOT_BYTES    bytes per slot, key and count included
//   HEADER_CELLS  cells that live in the header instead of a slot: cell capacity + j has the key CELL_EMPTY and its count in
//                 hdr[j] (overlap.hip: the one pair that equals the marker)
//   layout(t, capacity)        host: the pointers of Table behind the counts
//   clear(t, i)                device: the rest of slot i as reset leaves it
//   move(from, i, k, c, to)    device: cell i (key k, count c) into another table, through the family's *_global_add
//   write(t, i, out, pos)      device: the rest of slot i to output row pos
// The core owns the header, the keys and the counts; the count kernels and their probe loops stay with the family.
#pragma once
#include "label_stream.h"

namespace emp {

constexpr uint64_t CELL_EMPTY = ~0ull;
constexpr size_t CELL_HEADER = 64;

template <class F>
inline typename F::Table cells_table(void* d_table, int64_t capacity) {
  typename F::Table t;
  t.hdr = (uint64_t*)d_table;
  t.keys = (uint64_t*)((char*)d_table + CELL_HEADER);
  t.counts = t.keys + capacity;
  t.mask = (uint64_t)capacity - 1;
  F::layout(t, capacity);
  return t;
}

// key and count of cell i < capacity + HEADER_CELLS
template <class T>
__device__ __forceinline__ uint64_t cell_read(const T& t, int64_t capacity, int64_t i, uint64_t& key) {
  key = i < capacity ? t.keys[i] : CELL_EMPTY;
  if (i >= capacity) return t.hdr[i - capacity];
  return key != CELL_EMPTY ? t.counts[i] : 0;
}

template <class F>
__global__ void __launch_bounds__(256) label_cells_reset_kernel(typename F::Table t, int64_t capacity) {
  const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i0 < (int64_t)(CELL_HEADER / 8)) t.hdr[i0] = 0;
  for (int64_t i = i0; i < capacity; i += (int64_t)gridDim.x * 256) {
    t.keys[i] = CELL_EMPTY;
    t.counts[i] = 0;
    F::clear(t, i);
  }
}

// every cell of `from` into `to` (a larger table)
template <class F>
__global__ void __launch_bounds__(256) label_cells_rehash_kernel(typename F::Table from, int64_t capacity, typename F::Table to) {
  const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (int64_t i = i0; i < capacity + F::HEADER_CELLS; i += (int64_t)gridDim.x * 256) {
    uint64_t k;
    const uint64_t c = cell_read(from, capacity, i, k);
    if (c != 0) F::move(from, i, k, c, to);
  }
}

// the cells -> output rows in arrival order (the caller sorts); hdr[2] is the cursor, one atomic per wave
template <class F>
__global__ void __launch_bounds__(256) label_cells_compact_kernel(typename F::Table t, int64_t capacity, typename F::Out out, int64_t max_out) {
  const int lane = threadIdx.x & 63;
  const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * 256;
  const int64_t cells = capacity + F::HEADER_CELLS;
  const int64_t rounds = (cells + step - 1) / step;
  for (int64_t r = 0; r < rounds; ++r) {
    const int64_t i = i0 + r * step;
    uint64_t k = CELL_EMPTY;
    const uint64_t c = i < cells ? cell_read(t, capacity, i, k) : 0;
    const bool keep = c != 0;
    const uint64_t m = __ballot(keep);
    if (m == 0) continue;
    const int leader = __ffsll((unsigned long long)m) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd((unsigned long long*)&t.hdr[2], (unsigned long long)__popcll(m));
    base = __shfl(base, leader);
    if (keep) {
      const int64_t pos = (int64_t)base + __popcll(m & ((1ull << lane) - 1ull));
      if (pos < max_out) {
        out.keys[pos] = k;
        out.counts[pos] = c;
        F::write(t, i, out, pos);
      }
    }
  }
}

inline int cells_grid(int64_t items) {
  int64_t g = (items + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

inline bool cells_capacity_ok(int64_t c) { return c >= 64 && c <= (1ll << 32) && (c & (c - 1)) == 0; }

template <class F>
int cells_reset(void* d_table, int64_t capacity, hipStream_t s) {
  hipLaunchKernelGGL(label_cells_reset_kernel<F>, dim3(cells_grid(capacity)), dim3(256), 0, s, cells_table<F>(d_table, capacity), capacity);
  EMP_LAUNCH_CHECK();
  return EMP_OK;
}

// One slab into the table whose header is hdr.  count(negate) launches the family's count kernel over the slab; `entry` and
// `domain` word the error for a label outside the key's domain.  Synchronises the stream (it reads the table's flags).
// *h_overflow = 1: the table was too small for this slab; the same slab with negated weights has taken out again what the call
// had added.
template <class Count>
int cells_accumulate(uint64_t* hdr, hipStream_t s, const char* entry, const char* domain, Count count, int* h_overflow) {
  int rc = count(0);
  if (rc) return rc;
  uint32_t flags[2] = {0, 0};
  EMP_CHECK_HIP(hipMemcpyAsync(flags, &hdr[1], sizeof(flags), hipMemcpyDeviceToHost, s));
  EMP_CHECK_HIP(hipStreamSynchronize(s));
  EMP_REQUIRE(flags[1] == 0, "%s: a label outside %s", entry, domain);
  if (flags[0]) {
    rc = count(1);
    if (rc) return rc;
    EMP_CHECK_HIP(hipMemsetAsync(&hdr[1], 0, 8, s));
    EMP_CHECK_HIP(hipStreamSynchronize(s));
    *h_overflow = 1;
  }
  return EMP_OK;
}

// Moves the cells of a table into an empty (reset) larger one.  Synchronises; *h_overflow = 1: d_to is too small as well
// (reset it, or a larger one, and call again: d_from is unchanged).
template <class F>
int cells_grow(const void* d_from, int64_t from_capacity, void* d_to, int64_t to_capacity, hipStream_t s, int* h_overflow) {
  const typename F::Table to = cells_table<F>(d_to, to_capacity);
  hipLaunchKernelGGL(label_cells_rehash_kernel<F>, dim3(cells_grid(from_capacity + F::HEADER_CELLS)), dim3(256), 0, s,
                     cells_table<F>((void*)d_from, from_capacity), from_capacity, to);
  EMP_LAUNCH_CHECK();
  uint32_t flag = 0;
  EMP_CHECK_HIP(hipMemcpyAsync(&flag, &to.hdr[1], sizeof(flag), hipMemcpyDeviceToHost, s));
  EMP_CHECK_HIP(hipStreamSynchronize(s));
  *h_overflow = flag != 0;
  return EMP_OK;
}

// Synchronises.  *h_num = number of cells; the first min(*h_num, max_out) of them are written.
template <class F>
int cells_finalize(void* d_table, int64_t capacity, const typename F::Out& out, int64_t max_out, int64_t* h_num, hipStream_t s) {
  const typename F::Table t = cells_table<F>(d_table, capacity);
  EMP_CHECK_HIP(hipMemsetAsync(&t.hdr[2], 0, 8, s));
  hipLaunchKernelGGL(label_cells_compact_kernel<F>, dim3(cells_grid(capacity + F::HEADER_CELLS)), dim3(256), 0, s, t, capacity, out, max_out);
  EMP_LAUNCH_CHECK();
  uint64_t num = 0;
  EMP_CHECK_HIP(hipMemcpyAsync(&num, &t.hdr[2], 8, hipMemcpyDeviceToHost, s));
  EMP_CHECK_HIP(hipStreamSynchronize(s));
  *h_num = (int64_t)num;
  return EMP_OK;
}

}  // namespace emp
