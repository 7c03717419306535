// tvl1_fbcheck.hpp — kernels of the forward-backward consistency score.
//
// Given the forward flow (uf, vf) of a pair I0 -> I1 and the backward flow (ub, vb) of I1 -> I0,
// a px (x, y) follows its forward flow to (X, Y) = (x + uf, y + vf), reads the backward flow
// there (bilinear, the last tap clamped to the frame) and scores how far the two are from
// cancelling:
//
//   score = |f + b(X, Y)|^2 - alpha (|f|^2 + |b(X, Y)|^2),      +inf where (X, Y) leaves the frame
//
// so that "consistent at beta" is score <= beta (false for NaN and +inf) and one score plane
// serves any beta.  Every operation is one IEEE f32 rounding in the order of tests/fbcheck_ref.py
// (numpy), whatever the ctx's fast_math or profile: contraction is switched off in these
// functions themselves, not only by the build's flags.
//
//   k_fb_score     the score plane of every pair of a batch;
//   k_zero_above   u = v = 0 where !(score <= beta), and how many such px each pair has.
//
// The planes may be ROI views: any pointer and any pitch that are multiples of 4.  A lane owns 4
// adjacent px of a row and moves them as one 16-byte word where the row address allows, float by
// float otherwise; no float outside a row's w px is ever touched.  Included by tvl1_engine.hip
// only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tvl1_kernels.hpp"   // imin, imax

namespace tvl1k {

constexpr int kFbPx = 4;          // px of a row per lane
constexpr int kFbMaxRowGroups = 65535;   // grid z: a block then walks down the rows

struct FbScoreArgs {
  const float *uf, *vf;
  size_t fp, fs;          // forward planes: row pitch and pair stride (bytes)
  const float *ub, *vb;
  size_t bp, bs;          // backward planes
  int w, h;
  float alpha;
  float *score;
  size_t sp, ss;
};

// 4 floats of a row at r (k < n of them inside the row): one 16-byte word where r allows
__device__ __forceinline__ void fb_load4(const float *r, int n, float out[kFbPx]) {
  if (n == kFbPx && (reinterpret_cast<uintptr_t>(r) & 15) == 0) {
    const float4 t = *reinterpret_cast<const float4 *>(r);
    out[0] = t.x, out[1] = t.y, out[2] = t.z, out[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < kFbPx; ++k) out[k] = k < n ? r[k] : 0.0f;
  }
}

__device__ __forceinline__ void fb_store4(float *r, int n, const float in[kFbPx]) {
  if (n == kFbPx && (reinterpret_cast<uintptr_t>(r) & 15) == 0) {
    *reinterpret_cast<float4 *>(r) = make_float4(in[0], in[1], in[2], in[3]);
  } else {
#pragma unroll
    for (int k = 0; k < kFbPx; ++k)
      if (k < n) r[k] = in[k];
  }
}

// One plane's bilinear sample: exact at ax = 0 or ay = 0 as long as the other taps are finite
__device__ __forceinline__ float fb_sample(const char *P, size_t pitch, int x0, int x1, int y0, int y1,
                                           float ax, float ay) {
#pragma clang fp contract(off)
  const float *r0 = reinterpret_cast<const float *>(P + (size_t)y0 * pitch);
  const float *r1 = reinterpret_cast<const float *>(P + (size_t)y1 * pitch);
  const float p00 = r0[x0], p01 = r0[x1], p10 = r1[x0], p11 = r1[x1];
  const float t = p00 + ax * (p01 - p00);
  const float b = p10 + ax * (p11 - p10);
  return t + ay * (b - t);
}

// The score of a px whose landing point (X, Y) lies inside the frame (0 <= X <= w - 1, 0 <= Y
// <= h - 1: the conversions below are in range)
__device__ __forceinline__ float fb_score_px(const char *ub, const char *vb, size_t bp, int w, int h,
                                             float uf, float vf, float X, float Y, float alpha) {
#pragma clang fp contract(off)
  const float fx = floorf(X), fy = floorf(Y);
  const int x0 = (int)fx, y0 = (int)fy;
  const float ax = X - fx, ay = Y - fy;
  const int x1 = imin(x0 + 1, w - 1), y1 = imin(y0 + 1, h - 1);
  const float ubs = fb_sample(ub, bp, x0, x1, y0, y1, ax, ay);
  const float vbs = fb_sample(vb, bp, x0, x1, y0, y1, ax, ay);
  const float ex = uf + ubs, ey = vf + vbs;
  const float err = ex * ex + ey * ey;
  const float mag = (uf * uf + vf * vf) + (ubs * ubs + vbs * vbs);
  const float am = alpha * mag;
  return err - am;
}

// Grid (256-px tiles, pair, row groups), block 64 x 4: a lane owns 4 adjacent px of a row, a
// wavefront 256 px of it, and walks down the rows 4 gridDim.z apart (one step unless h is
// above 4 x 65535).  The eight backward taps of a px are gathered from global memory: flows are
// a few px, so neighbouring lanes' taps share cache lines.  A wavefront none of whose px lands
// inside the frame (a flow that points out of it everywhere) skips the gather as a whole: one
// scalar branch; inside it a px that lands outside converts nothing and reads no tap.
__global__ __launch_bounds__(256) void k_fb_score(FbScoreArgs a) {
#pragma clang fp contract(off)
  const int pair = __builtin_amdgcn_readfirstlane(blockIdx.y);
  const int x = (blockIdx.x * 64 + threadIdx.x) * kFbPx;
  if (x >= a.w) return;
  const int n = imin(kFbPx, a.w - x);
  const char *uf = reinterpret_cast<const char *>(a.uf) + (size_t)pair * a.fs;
  const char *vf = reinterpret_cast<const char *>(a.vf) + (size_t)pair * a.fs;
  const char *ub = reinterpret_cast<const char *>(a.ub) + (size_t)pair * a.bs;
  const char *vb = reinterpret_cast<const char *>(a.vb) + (size_t)pair * a.bs;
  char *sc = reinterpret_cast<char *>(a.score) + (size_t)pair * a.ss;
  const float xmax = (float)(a.w - 1), ymax = (float)(a.h - 1);
  const int ystep = (int)gridDim.z * 4;
  for (int y = blockIdx.z * 4 + threadIdx.y; y < a.h; y += ystep) {
    float u[kFbPx], v[kFbPx], X[kFbPx], s[kFbPx];
    fb_load4(reinterpret_cast<const float *>(uf + (size_t)y * a.fp) + x, n, u);
    fb_load4(reinterpret_cast<const float *>(vf + (size_t)y * a.fp) + x, n, v);
    bool in[kFbPx], any = false;
    float Y[kFbPx];
#pragma unroll
    for (int k = 0; k < kFbPx; ++k) {
      X[k] = (float)(x + k) + u[k];
      Y[k] = (float)y + v[k];
      // false for NaN
      in[k] = k < n && X[k] >= 0.0f && X[k] <= xmax && Y[k] >= 0.0f && Y[k] <= ymax;
      any |= in[k];
      s[k] = __builtin_inff();
    }
    if (__builtin_amdgcn_ballot_w64(any) != 0) {   // wavefront-uniform
#pragma unroll
      for (int k = 0; k < kFbPx; ++k)
        if (in[k]) s[k] = fb_score_px(ub, vb, a.bp, a.w, a.h, u[k], v[k], X[k], Y[k], a.alpha);
    }
    fb_store4(reinterpret_cast<float *>(sc + (size_t)y * a.sp) + x, n, s);
  }
}

struct ZeroAboveArgs {
  float *u, *v;
  size_t fp, fs;          // flow planes: row pitch and pair stride (bytes)
  const float *score;
  size_t sp, ss;
  int w, h;
  float beta;
  unsigned long long *count;   // per pair, zero before the launch; NULL: not counted
};

// u = v = 0 where !(score <= beta): the I1 <= 1 mask's sibling.  Grid and ownership as
// k_fb_score's.  A lane none of whose px is rejected touches neither flow plane.  Rejected px
// per pair: per-lane u32 partials (a lane meets at most 4 px a row and 2^24 / (4 x 65535) + 1
// rows), a wavefront sum, and one u64 atomicAdd per block (integer: any order, one total).
__global__ __launch_bounds__(256) void k_zero_above(ZeroAboveArgs a) {
  const int pair = __builtin_amdgcn_readfirstlane(blockIdx.y);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
  const int x = (blockIdx.x * 64 + threadIdx.x) * kFbPx;
  const int n = imax(0, imin(kFbPx, a.w - x));
  char *up = reinterpret_cast<char *>(a.u) + (size_t)pair * a.fs;
  char *vp = reinterpret_cast<char *>(a.v) + (size_t)pair * a.fs;
  const char *sc = reinterpret_cast<const char *>(a.score) + (size_t)pair * a.ss;
  const int ystep = (int)gridDim.z * 4;
  uint32_t cnt = 0;
  if (n > 0) {
    for (int y = blockIdx.z * 4 + wv; y < a.h; y += ystep) {
      float s[kFbPx];
      fb_load4(reinterpret_cast<const float *>(sc + (size_t)y * a.sp) + x, n, s);
      bool rej[kFbPx], any = false;
#pragma unroll
      for (int k = 0; k < kFbPx; ++k) {
        rej[k] = k < n && !(s[k] <= a.beta);   // NaN and +inf are rejected
        any |= rej[k];
        cnt += rej[k] ? 1u : 0u;
      }
      if (!any) continue;
      float *ur = reinterpret_cast<float *>(up + (size_t)y * a.fp) + x;
      float *vr = reinterpret_cast<float *>(vp + (size_t)y * a.fp) + x;
      if (n == kFbPx && ((reinterpret_cast<uintptr_t>(ur) | reinterpret_cast<uintptr_t>(vr)) & 15) == 0) {
        float4 tu = *reinterpret_cast<const float4 *>(ur), tv = *reinterpret_cast<const float4 *>(vr);
        if (rej[0]) tu.x = 0.0f, tv.x = 0.0f;
        if (rej[1]) tu.y = 0.0f, tv.y = 0.0f;
        if (rej[2]) tu.z = 0.0f, tv.z = 0.0f;
        if (rej[3]) tu.w = 0.0f, tv.w = 0.0f;
        *reinterpret_cast<float4 *>(ur) = tu;
        *reinterpret_cast<float4 *>(vr) = tv;
      } else {
#pragma unroll
        for (int k = 0; k < kFbPx; ++k)
          if (rej[k]) ur[k] = 0.0f, vr[k] = 0.0f;
      }
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
