// tvl1_score.hpp — kernels of the photometric (ZNCC) score of a flow.
//
// Given the two u8 frames of a pair and its forward flow (u, v), I1(x + u, y + v) ~ I0(x, y):
//
//   step 1  J = frame1 warped back along the flow, sampled as k_remap_flow_u8 samples (the map
//           rounded to 1/32 px, 5-bit weights, integer blend), and m = the landing point lies
//           inside the frame (false for NaN); where !m nothing is converted and no tap is read;
//   step 2  over the (2R+1)^2 window cut to the frame and to px with m: n, Sa = sum I0, Sb = sum J,
//           Saa, Sbb, Sab, then A = n Sab - Sa Sb, B = n Saa - Sa^2, C = n Sbb - Sb^2: integers,
//           below 2^29, exact in any order;
//   step 3  score = float(1.0 - double(A) / sqrt(double(B) * double(C))), +inf where the centre
//           has !m or B == 0 or C == 0: four IEEE f64 operations and one conversion, each rounded
//           once whatever the ctx's fast_math or profile (tests/zncc_ref.py restates all of it).
//
//   k_zncc_score<R>   the score plane of every pair of a batch, R = 1..4;
//   k_warp_flow_u8    step 1 alone: J (0 where !m) and, optionally, m as a 0/1 plane.
//
// Both call zn_warp_px, so a test of the second pins the sample the first one scores.  The
// frames may be ROI views of any pointer and pitch, the f32 planes of any pointer and pitch that
// are multiples of 4; nothing outside a row's w px or a plane's h rows is ever read.  Included by
// tvl1_engine.hip only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tvl1_fbcheck.hpp"   // fb_load4
#include "tvl1_kernels.hpp"   // imin, imax

namespace tvl1k {

constexpr int kZnSegRows = 64;        // rows of a segment: one wavefront walks down them
constexpr int kZnMaxRowGroups = 65535;   // k_warp_flow_u8's grid z: a block then walks down the rows

// Step 1 for one px: true iff it lands inside the frame, J its sample then (0 otherwise).  Inside,
// 0 <= mx <= w - 1 <= 2^19: mx * 32 is an exact integer below 2^24 after rint, sx <= w - 1, and
// sx = w - 1 comes with fx = 0, so the clamped tap x1 carries weight 0 (rows likewise).
__device__ __forceinline__ bool zn_warp_px(const uint8_t *I1, size_t pitch, int w, int h, int x, int y,
                                           float u, float v, int &J) {
#pragma clang fp contract(off)
  const float mx = (float)x + u, my = (float)y + v;
  J = 0;
  if (!(mx >= 0.0f && mx <= (float)(w - 1) && my >= 0.0f && my <= (float)(h - 1))) return false;   // NaN too
  const int ix = (int)rintf(mx * 32.f), iy = (int)rintf(my * 32.f);
  const int sx = ix >> 5, fx = ix & 31, sy = iy >> 5, fy = iy & 31;
  const int x1 = imin(sx + 1, w - 1), y1 = imin(sy + 1, h - 1);
  const uint8_t *r0 = I1 + (size_t)sy * pitch, *r1 = I1 + (size_t)y1 * pitch;
  const int s00 = r0[sx], s01 = r0[x1], s10 = r1[sx], s11 = r1[x1];
  J = (s00 * (32 - fx) * (32 - fy) + s01 * fx * (32 - fy) + s10 * (32 - fx) * fy + s11 * fx * fy + 512) >> 10;
  return true;
}

struct ZnccArgs {
  const uint8_t *I0, *I1;
  size_t p0, s0, p1, s1;   // frames: row pitch and pair stride (bytes; stride 0: one shared frame)
  const float *u, *v;
  size_t fp, fs;           // flow planes
  int w, h;
  float *score;
  size_t sp, ss;
};

// A px is kept packed as I0 | J << 8 | m << 16 (0 where !m: such a px adds nothing to any sum).
// Its six sums travel in four words whose fields cannot carry into each other up to a 9 x 9
// window: Sa | Sb << 16 (<= 81 x 255 < 2^15 each), Saa | n << 24 (<= 81 x 255^2 < 2^23, n < 2^7),
// Sbb, Sab.  Adding a px and taking one away again are field-wise exact.
struct ZnSums {
  uint32_t w0, w1, w2, w3;
};

__device__ __forceinline__ void zn_terms(uint32_t p, ZnSums &t) {
  const uint32_t a = p & 255u, b = (p >> 8) & 255u, m = p >> 16;
  t.w0 = a | b << 16;
  t.w1 = a * a | m << 24;
  t.w2 = b * b;
  t.w3 = a * b;
}

__device__ __forceinline__ uint32_t zn_lane(uint32_t v, int lane) {   // v of lane `lane` mod 64
  return (uint32_t)__builtin_amdgcn_ds_bpermute((lane & 63) << 2, (int)v);
}

// Grid (bands / 4, segments, pairs), block 64 x 4.  A wavefront owns a band of 64 - 2R output
// columns of one segment of kZnSegRows rows; its 64 lanes are the band's columns and R halo
// columns either side, lane = column.  It walks down from R rows above the segment to R rows
// below it: per row a lane makes its column's packed px once (rows and columns outside the frame
// give 0), adds it to the column's sums of the last 2R+1 rows and takes the leaving row's away
// (the ring of packed px is in registers, the products are recomputed: integers, exact), then
// the 2R+1 neighbouring columns' sums are added across lanes and the centre row's score is
// stored.  Halo columns and run-in rows are recomputed by the neighbouring wavefronts and never
// stored.  The next row's flow is loaded before this row's taps, so one latency hides the other.
// The f64 tail runs only where the centre is valid and B, C > 0.
template <int R>
__global__ __launch_bounds__(256) void k_zncc_score(ZnccArgs a) {
#pragma clang fp contract(off)
  constexpr int D = 2 * R + 1, BW = 64 - 2 * R;
  const int pair = __builtin_amdgcn_readfirstlane(blockIdx.z);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
  const int xb = (blockIdx.x * 4 + wv) * BW;   // the band's first output column
  if (xb >= a.w) return;                       // the whole wavefront; no barrier below
  const int lane = threadIdx.x;
  const int c = xb - R + lane;
  const bool cin = c >= 0 && c < a.w;
  const bool owns = lane >= R && lane < 64 - R && c < a.w;
  const int y0 = blockIdx.y * kZnSegRows, y1 = imin(y0 + kZnSegRows, a.h);
  const uint8_t *I0 = a.I0 + (size_t)pair * a.s0;
  const uint8_t *I1 = a.I1 + (size_t)pair * a.s1;
  const char *up = reinterpret_cast<const char *>(a.u) + (size_t)pair * a.fs;
  const char *vp = reinterpret_cast<const char *>(a.v) + (size_t)pair * a.fs;
  char *sc = reinterpret_cast<char *>(a.score) + (size_t)pair * a.ss;

  uint32_t ring[D];
#pragma unroll
  for (int k = 0; k < D; ++k) ring[k] = 0;
  ZnSums cs{0, 0, 0, 0};
  const int ya = imax(y0 - R, 0), yb = imin(y1 + R, a.h);   // rows that exist
  float un = 0.0f, vn = 0.0f;
  if (cin) {
    un = reinterpret_cast<const float *>(up + (size_t)ya * a.fp)[c];
    vn = reinterpret_cast<const float *>(vp + (size_t)ya * a.fp)[c];
  }
  for (int yy = y0 - R; yy < y1 + R; ++yy) {
    uint32_t p = 0;
    if (yy >= ya && yy < yb) {   // wavefront-uniform
      const float u = un, v = vn;
      if (cin && yy + 1 < yb) {
        un = reinterpret_cast<const float *>(up + (size_t)(yy + 1) * a.fp)[c];
        vn = reinterpret_cast<const float *>(vp + (size_t)(yy + 1) * a.fp)[c];
      }
      int J;
      if (cin && zn_warp_px(I1, a.p1, a.w, a.h, c, yy, u, v, J))
        p = (uint32_t)I0[(size_t)yy * a.p0 + c] | (uint32_t)J << 8 | 1u << 16;
    }
    ZnSums in, out;
    zn_terms(p, in);
    zn_terms(ring[0], out);
    cs.w0 += in.w0 - out.w0, cs.w1 += in.w1 - out.w1, cs.w2 += in.w2 - out.w2, cs.w3 += in.w3 - out.w3;
#pragma unroll
    for (int k = 0; k + 1 < D; ++k) ring[k] = ring[k + 1];
    ring[D - 1] = p;
    const int yo = yy - R;       // the row whose window is now complete: ring[R]
    if (yo < y0) continue;       // run-in (wavefront-uniform)
    ZnSums hs = cs;
#pragma unroll
    for (int d = 1; d <= R; ++d) {
      hs.w0 += zn_lane(cs.w0, lane - d) + zn_lane(cs.w0, lane + d);
      hs.w1 += zn_lane(cs.w1, lane - d) + zn_lane(cs.w1, lane + d);
      hs.w2 += zn_lane(cs.w2, lane - d) + zn_lane(cs.w2, lane + d);
      hs.w3 += zn_lane(cs.w3, lane - d) + zn_lane(cs.w3, lane + d);
    }
    if (!owns) continue;         // halo lanes hold other lanes' wrapped sums: never used
    float s = __builtin_inff();
    if (ring[R] >> 16) {
      const int n = (int)(hs.w1 >> 24), Sa = (int)(hs.w0 & 0xffffu), Sb = (int)(hs.w0 >> 16);
      const int Saa = (int)(hs.w1 & 0xffffffu), Sbb = (int)hs.w2, Sab = (int)hs.w3;
      // all three below 2^29: 81^2 x 255^2 = 4.27e8
      const int A = n * Sab - Sa * Sb, B = n * Saa - Sa * Sa, C = n * Sbb - Sb * Sb;
      if (B != 0 && C != 0) {
        const double bc = (double)B * (double)C;
        const double q = (double)A / sqrt(bc);
        s = (float)(1.0 - q);
      }
    }
    reinterpret_cast<float *>(sc + (size_t)yo * a.sp)[c] = s;
  }
}

struct WarpFlowArgs {
  const uint8_t *I1;
  size_t p1;
  const float *u, *v;
  size_t fp;
  int w, h;
  uint8_t *dst;
  size_t dp;
  uint8_t *valid;   // or NULL
  size_t vp;
};

__device__ __forceinline__ void zn_store4(uint8_t *d, int n, const uint32_t b[4]) {
  if (n == 4 && (reinterpret_cast<uintptr_t>(d) & 3) == 0) {
    *reinterpret_cast<uint32_t *>(d) = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n) d[k] = (uint8_t)b[k];
  }
}

// Step 1 as a plane: grid and ownership as k_fb_score's (a lane owns 4 adjacent px of a row, a
// block walks down the rows 4 gridDim.z apart).
__global__ __launch_bounds__(256) void k_warp_flow_u8(WarpFlowArgs a) {
#pragma clang fp contract(off)
  const int x = (blockIdx.x * 64 + threadIdx.x) * kFbPx;
  if (x >= a.w) return;
  const int n = imin(kFbPx, a.w - x);
  const int ystep = (int)gridDim.z * 4;
  for (int y = blockIdx.z * 4 + threadIdx.y; y < a.h; y += ystep) {
    float u[kFbPx], v[kFbPx];
    fb_load4(reinterpret_cast<const float *>(reinterpret_cast<const char *>(a.u) + (size_t)y * a.fp) + x, n, u);
    fb_load4(reinterpret_cast<const float *>(reinterpret_cast<const char *>(a.v) + (size_t)y * a.fp) + x, n, v);
    uint32_t J[kFbPx], m[kFbPx];
#pragma unroll
    for (int k = 0; k < kFbPx; ++k) {
      int j = 0;
      m[k] = k < n && zn_warp_px(a.I1, a.p1, a.w, a.h, x + k, y, u[k], v[k], j) ? 1u : 0u;
      J[k] = (uint32_t)j;
    }
    zn_store4(a.dst + (size_t)y * a.dp + x, n, J);
    if (a.valid) zn_store4(a.valid + (size_t)y * a.vp + x, n, m);
  }
}

}  // namespace tvl1k
