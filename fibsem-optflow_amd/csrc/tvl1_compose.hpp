// tvl1_compose.hpp — the kernel of flow composition.
//
// Given the flow a = (ua, va) of a pair A -> B and the flow b = (ub, vb) of B -> C, a px (x, y)
// follows a to (X, Y) = (x + ua, y + va), reads b there (bilinear, fb_sample's arithmetic) and
// adds the two:
//
//   c(x) = a(x) + b(x + a(x))
//
// is the flow A -> C.  A landing point outside the frame is clamped to it (NaN and -inf to 0, +inf
// to the far edge) and counted, so no tap is ever read outside the plane whatever the input; a
// NaN or an infinity in a or b propagates into c and never becomes an address.  Every float
// operation is one IEEE f32 rounding in the order of tests/compose_ref.py (numpy), whatever the
// ctx's fast_math or profile: contraction is switched off in the function itself, not only by the
// build's flags.
//
// The planes may be ROI views, with k_fb_score's ownership: a lane owns 4 adjacent px of a row
// and moves them as one 16-byte word where the row address allows, float by float otherwise; no
// float outside a row's w px is ever touched.  c may be a itself (a px reads its own a and nobody
// else's), never b.  Included by tvl1_engine.hip only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tvl1_fbcheck.hpp"   // kFbPx, fb_load4, fb_store4, fb_sample

namespace tvl1k {

struct ComposeArgs {
  const float *ua, *va;
  size_t ap, as;          // flow A -> B: row pitch and pair stride (bytes)
  const float *ub, *vb;
  size_t bp, bs;          // flow B -> C
  int w, h;
  float *uc, *vc;
  size_t cp, cs;          // flow A -> C
  unsigned long long *count;   // per pair, zero before the launch; NULL: not counted
};

// Grid and ownership as k_fb_score's: (256-px tiles, pair, row groups), block 64 x 4, rows walked
// 4 gridDim.z apart.  The eight taps of a px are gathered from global memory.  Px that land
// outside the frame, per pair: k_zero_above's pattern (per-lane u32 partials, a wavefront sum,
// four wavefronts through LDS, one u64 atomicAdd per block; integer: any order, one total).
__global__ __launch_bounds__(256) void k_compose_flow(ComposeArgs a) {
#pragma clang fp contract(off)
  const int pair = __builtin_amdgcn_readfirstlane(blockIdx.y);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
  const int x = (blockIdx.x * 64 + threadIdx.x) * kFbPx;
  const int n = imax(0, imin(kFbPx, a.w - x));
  const char *ua = reinterpret_cast<const char *>(a.ua) + (size_t)pair * a.as;
  const char *va = reinterpret_cast<const char *>(a.va) + (size_t)pair * a.as;
  const char *ub = reinterpret_cast<const char *>(a.ub) + (size_t)pair * a.bs;
  const char *vb = reinterpret_cast<const char *>(a.vb) + (size_t)pair * a.bs;
  char *uc = reinterpret_cast<char *>(a.uc) + (size_t)pair * a.cs;
  char *vc = reinterpret_cast<char *>(a.vc) + (size_t)pair * a.cs;
  const float xmax = (float)(a.w - 1), ymax = (float)(a.h - 1);
  const int ystep = (int)gridDim.z * 4;
  uint32_t cnt = 0;
  if (n > 0) {
    for (int y = blockIdx.z * 4 + wv; y < a.h; y += ystep) {
      float u[kFbPx], v[kFbPx], cu[kFbPx], cv[kFbPx];
      fb_load4(reinterpret_cast<const float *>(ua + (size_t)y * a.ap) + x, n, u);
      fb_load4(reinterpret_cast<const float *>(va + (size_t)y * a.ap) + x, n, v);
#pragma unroll
      for (int k = 0; k < kFbPx; ++k) {
        cu[k] = cv[k] = 0.0f;
        if (k >= n) continue;
        const float X = (float)(x + k) + u[k];
        const float Y = (float)y + v[k];
        // false for NaN
        const bool inside = X >= 0.0f && X <= xmax && Y >= 0.0f && Y <= ymax;
        cnt += inside ? 0u : 1u;
        // NaN and -inf give 0, +inf the far edge: the conversions below are in range
        const float Xc = X >= 0.0f ? (X <= xmax ? X : xmax) : 0.0f;
        const float Yc = Y >= 0.0f ? (Y <= ymax ? Y : ymax) : 0.0f;
        const float fx = floorf(Xc), fy = floorf(Yc);
        const int x0 = (int)fx, y0 = (int)fy;
        const float ax = Xc - fx, ay = Yc - fy;
        const int x1 = imin(x0 + 1, a.w - 1), y1 = imin(y0 + 1, a.h - 1);
        const float ubs = fb_sample(ub, a.bp, x0, x1, y0, y1, ax, ay);
        const float vbs = fb_sample(vb, a.bp, x0, x1, y0, y1, ax, ay);
        cu[k] = u[k] + ubs;
        cv[k] = v[k] + vbs;
      }
      fb_store4(reinterpret_cast<float *>(uc + (size_t)y * a.cp) + x, n, cu);
      fb_store4(reinterpret_cast<float *>(vc + (size_t)y * a.cp) + x, n, cv);
    }
  }
  if (!a.count) return;   // a kernel argument: the whole block leaves
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  __shared__ uint32_t red[4];
  if (threadIdx.x == 0) red[wv] = cnt;
  __syncthreads();
  if (threadIdx.x == 0 && threadIdx.y == 0) {
    const unsigned long long t = (unsigned long long)red[0] + red[1] + red[2] + red[3];
    if (t) atomicAdd(a.count + pair, t);
  }
}

}  // namespace tvl1k
