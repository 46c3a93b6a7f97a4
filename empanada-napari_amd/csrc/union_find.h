// Lock-free union-find on linear voxel indices, shared by the connected components of equal labels (sparse.hip) and the
// background components of Fill holes (morph.hip).  A root is the smallest index of its component; linking is one atomicMin,
// so the result does not depend on the order of the unions.
#pragma once
#include <hip/hip_runtime.h>

namespace emp {

// parent words are read past the per-CU L1 (agent-scope relaxed loads): other workgroups update them
// with atomicMin while this one walks the tree
__device__ __forceinline__ int uf_load(int* parent, int a) {
  return __hip_atomic_load(&parent[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int uf_find(int* parent, int a) {
  int p = uf_load(parent, a);
  while (p != a) {
    a = p;
    p = uf_load(parent, a);
  }
  return a;
}
__device__ __forceinline__ void uf_union(int* parent, int a, int b) {
  while (true) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) { int t = a; a = b; b = t; }   // a > b: hang the larger root under the smaller
    int old = atomicMin(&parent[a], b);
    if (old == a) return;
    a = old;
  }
}

}  // namespace emp
