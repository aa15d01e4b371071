// rc2dgi_launch.h -- what the pass units' launchers share (internal: only the .hip units include it).
#pragma once

#include <hip/hip_runtime.h>

namespace rc2dgi {

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// 256-thread workgroups of 64 x 4 texels
static inline dim3 grid2d(int w, int h) { return dim3(ceil_div(w, 64), ceil_div(h, 4)); }

// rows [row0, row1) of n, row1 = -1: all
static inline void clamp_rows(int n, int &row0, int &row1) {
  if (row1 < 0 || row1 > n) row1 = n;
  if (row0 < 0) row0 = 0;
}

// physical workgroup id -> logical id: every XCD (own L2) a contiguous chunk of the logical order
__host__ __device__ __forceinline__ int xcd_logical_id(int p, int n) {
  const int q = n >> 3, r = n & 7, x = p & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (p >> 3);
}

}  // namespace rc2dgi
