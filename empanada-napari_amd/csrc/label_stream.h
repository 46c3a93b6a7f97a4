// What the streaming kernels over label arrays share in their hot loops (overlap.hip, labels.hip, measure.hip): the hash of
// their open-addressing tables, the load of E consecutive elements of 1, 2, 4 or 8 bytes as raw unsigned values, the division
// that turns a raster offset into coordinates, the domain check of a one-label key and the min / max update of a cell's box.
// Everything here is inlined into the count kernels; what they share outside them -- the table itself -- is label_table.h.
#pragma once
#include "common.h"

namespace emp {

__host__ __device__ __forceinline__ uint64_t ov_hash(uint64_t k) {      // the 64-bit finaliser of MurmurHash3 (public domain)
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

template <int BYTES> struct OvVec;
template <> struct OvVec<16> { typedef uint4 type; };
template <> struct OvVec<8> { typedef uint2 type; };
template <> struct OvVec<4> { typedef uint32_t type; };
template <> struct OvVec<2> { typedef uint16_t type; };
template <int S> struct OvElem;
template <> struct OvElem<1> { typedef uint8_t type; };
template <> struct OvElem<2> { typedef uint16_t type; };
template <> struct OvElem<4> { typedef uint32_t type; };
template <> struct OvElem<8> { typedef uint64_t type; };

// a vector of E elements of S bytes <-> E raw unsigned values
template <int S, int E>
__device__ __forceinline__ void ov_unpack(const typename OvVec<S * E>::type& vec, uint64_t* v) {
  typename OvElem<S>::type e[E];
  __builtin_memcpy(e, &vec, sizeof(vec));
#pragma unroll
  for (int j = 0; j < E; ++j) v[j] = (uint64_t)e[j];
}

template <int S, int E>
__device__ __forceinline__ typename OvVec<S * E>::type ov_pack(const uint64_t* v) {
  typedef typename OvElem<S>::type T;
  T e[E];
#pragma unroll
  for (int j = 0; j < E; ++j) e[j] = (T)v[j];
  typename OvVec<S * E>::type vec;
  __builtin_memcpy(&vec, e, sizeof(vec));
  return vec;
}

// E elements of S bytes from element i0 on as raw unsigned values; nv of them exist (the rest read as 0).  One vector
// load where the base is aligned for it and the lane is full, element loads otherwise (the tail, a misaligned view).
template <int S, int E>
__device__ __forceinline__ void ov_load(const void* base, int64_t i0, int nv, int vec_ok, uint64_t* v) {
  typedef typename OvElem<S>::type T;
  typedef typename OvVec<S * E>::type V;
  const T* p = (const T*)base + i0;
  if (vec_ok && nv == E) {
    ov_unpack<S, E>(*(const V*)p, v);
  } else {
#pragma unroll
    for (int j = 0; j < E; ++j) v[j] = j < nv ? (uint64_t)p[j] : 0ull;
  }
}

// the counterpart: the low S bytes of v[0..nv) to elements i0.. (one vector store under the same conditions)
template <int S, int E>
__device__ __forceinline__ void ov_store(void* base, int64_t i0, int nv, int vec_ok, const uint64_t* v) {
  typedef typename OvElem<S>::type T;
  typedef typename OvVec<S * E>::type V;
  T* p = (T*)base + i0;
  if (vec_ok && nv == E) {
    *(V*)p = ov_pack<S, E>(v);
  } else {
#pragma unroll
    for (int j = 0; j < E; ++j)
      if (j < nv) p[j] = (T)v[j];
  }
}

// x / d for x < d + 2^13 (d < 2^31 - 2^13) from the float reciprocal of d: the estimate is off by one at most
__device__ __forceinline__ uint32_t ov_div(uint32_t x, uint32_t d, float inv, uint32_t& rem) {
  uint32_t q = (uint32_t)((float)x * inv);
  int32_t r = (int32_t)(x - q * d);
  if (r < 0) {
    --q;
    r += (int32_t)d;
  } else if ((uint32_t)r >= d) {
    ++q;
    r -= (int32_t)d;
  }
  rem = (uint32_t)r;
  return q;
}

// offset o (<= 2^12) from the voxel (bz, by, bx) in raster order; c: a kernel's context with H, W and their float reciprocals
template <class Ctx>
__device__ __forceinline__ void ov_coord(const Ctx& c, uint32_t bx, uint32_t by, uint32_t bz, uint32_t o, uint32_t& x, uint32_t& y, uint32_t& z) {
  x = bx + o;
  y = by;
  z = bz;
  if (x >= c.W) {
    y += ov_div(x, c.W, c.invW, x);
    if (y >= c.H) z += ov_div(y, c.H, c.invH, y);
  }
}

// values outside the domain of a key that holds one label: [0, 2^63) for the whole volume, [0, 2^32) per slice
template <int S>
__device__ __forceinline__ bool ov_key_out_of_range(uint64_t v, int is_signed, int per_slice) {
  if (S == 8) return per_slice ? (v >> 32) != 0 : (v >> 63) != 0;
  return is_signed && ((v >> (8 * S - 1)) & 1);
}

// the box r (lo[3], hi[3]: z, y, x, inclusive) into the six fields b of a cell in global memory.  A field is read before it is
// updated: a box converges after a few runs of its label
template <class R>
__device__ __forceinline__ void ov_box_update_global(uint32_t* b, const R& r) {
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    if (r.lo[f] < __hip_atomic_load(&b[f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&b[f], r.lo[f]);
    if (r.hi[f] > __hip_atomic_load(&b[3 + f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&b[3 + f], r.hi[f]);
  }
}

}  // namespace emp
