// What the streaming kernels over label arrays share (overlap.hip, labels.hip, measure.hip): the hash of their open-addressing
// tables, the load of E consecutive elements of 1, 2, 4 or 8 bytes as raw unsigned values, and the division that turns a raster
// offset into coordinates.
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

}  // namespace emp
