// tvl1_stack.hpp — kernels of the average-flow alignment of a slice list (style 2).
//
// For slice i of a stack: B = blend6 of the six neighbours, flow = TV-L1(F_i -> B) at the
// pre-scaled size, aligned = remap(F_i, flow).  The solver is the engine's own; these are the
// three memory-streaming stages around it, all on u8 planes with byte pitches:
//
//   k_blend6_u8      six pitched u8 planes -> their Gaussian-weighted mean, rounded half-to-even;
//   k_half_u8        the 2x2 mean (a + b + c + d + 2) >> 2 of a plane with even sizes (what
//                    cv::resize does to u8 at an exact 1/2 scale);
//   k_remap_flow_u8  the flow brought to the frame's size (bilinear, as k_resize_hp), times the
//                    gain, turned into a 1/32-px map and sampled with cv::remap's INTER_LINEAR
//                    on u8 (BORDER_CONSTANT 0) -- one kernel, so the full-size flow and map
//                    never exist in memory.
//
// Everything after the map's quantisation is integer arithmetic, and the blend is exact in 64-bit
// integers, so tests/avgflow_ref.py (numpy) and these kernels agree bit for bit.  [OCV] the
// remap restates OpenCV's fixed-point INTER_LINEAR from memory, unpinned like SURVEY Appendix A.
//
// A lane takes 8 (blend, half) or 4 (remap) adjacent px of one row and moves them as one 8-
// or 4-byte word when the row address allows it (the caller's planes may be ROI views: any
// pointer, any pitch), byte by byte otherwise.  Included by tvl1_engine.hip only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tvl1_kernels.hpp"   // imin, imax, round_map

namespace tvl1k {

// The blend's weights: float(float(exp(-d^2 / 4)) * s), d = 3, 2, 1, s = 0.5 / (e3 + e2 + e1)
// in double (cv::Vec6f times a double).  Each is a multiple of 2^-28 and the six sum to 1.
constexpr float kBlendW0 = 0x1.58cc7p-5f;    // neighbours at distance 3
constexpr float kBlendW1 = 0x1.2cddc8p-3f;   // ... 2
constexpr float kBlendW2 = 0x1.3e778ep-2f;   // ... 1
constexpr int kBlendShift = 28;
constexpr uint32_t kBlendI0 = (uint32_t)(kBlendW0 * 268435456.0f);
constexpr uint32_t kBlendI1 = (uint32_t)(kBlendW1 * 268435456.0f);
constexpr uint32_t kBlendI2 = (uint32_t)(kBlendW2 * 268435456.0f);
static_assert((float)kBlendI0 == kBlendW0 * 268435456.0f && (float)kBlendI1 == kBlendW1 * 268435456.0f &&
                  (float)kBlendI2 == kBlendW2 * 268435456.0f,
              "the blend weights are multiples of 2^-28");
static_assert(2ull * ((unsigned long long)kBlendI0 + kBlendI1 + kBlendI2) == 1ull << kBlendShift,
              "the blend weights sum to 1");

constexpr int kStackPx = 8;   // px per lane of k_blend6_u8 and k_half_u8 (outputs)
constexpr int kRemapPx = 4;   // px per lane of k_remap_flow_u8

struct Blend6Args {
  const uint8_t *f[6];
  size_t pitch[6];
};

// n <= 8 bytes of a row from p (n == 8 and p 8-byte aligned: one load)
__device__ __forceinline__ void load_row8(const uint8_t *p, int n, uint8_t (&o)[8]) {
  if (n == 8 && (reinterpret_cast<uintptr_t>(p) & 7) == 0) {
    const uint2 t = *reinterpret_cast<const uint2 *>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      o[k] = (uint8_t)(t.x >> (8 * k));
      o[4 + k] = (uint8_t)(t.y >> (8 * k));
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = k < n ? p[k] : (uint8_t)0;
  }
}

__device__ __forceinline__ void store_row8(uint8_t *p, int n, const uint32_t (&o)[8]) {
  if (n == 8 && (reinterpret_cast<uintptr_t>(p) & 7) == 0) {
    uint2 t;
    t.x = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;
    t.y = o[4] | o[5] << 8 | o[6] << 16 | o[7] << 24;
    *reinterpret_cast<uint2 *>(p) = t;
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < n) p[k] = (uint8_t)o[k];
  }
}

// B = saturate_u8(round-half-even(sum_k w_k F_k)): the sum in units of 2^-28 is an integer
// below 2^36 (exactly what a double accumulator holds), rounded once.
__global__ void k_blend6_u8(Blend6Args a, int W, int H, uint8_t *__restrict__ dst, size_t dp) {
  const int x = (blockIdx.x * 64 + threadIdx.x) * kStackPx;
  const int y = blockIdx.y * 4 + threadIdx.y;
  if (x >= W || y >= H) return;
  const int n = imin(kStackPx, W - x);
  const uint32_t wi[6] = {kBlendI0, kBlendI1, kBlendI2, kBlendI2, kBlendI1, kBlendI0};
  unsigned long long acc[kStackPx] = {};
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    uint8_t px[8];
    load_row8(a.f[k] + (size_t)y * a.pitch[k] + x, n, px);
#pragma unroll
    for (int j = 0; j < kStackPx; ++j) acc[j] += (unsigned long long)wi[k] * px[j];
  }
  uint32_t out[kStackPx];
#pragma unroll
  for (int j = 0; j < kStackPx; ++j) {
    uint32_t q = (uint32_t)(acc[j] >> kBlendShift);
    const uint32_t r = (uint32_t)acc[j] & ((1u << kBlendShift) - 1), half = 1u << (kBlendShift - 1);
    q += (r > half || (r == half && (q & 1u))) ? 1u : 0u;
    out[j] = q > 255u ? 255u : q;
  }
  store_row8(dst + (size_t)y * dp + x, n, out);
}

// dst(x, y) = (s(2x, 2y) + s(2x+1, 2y) + s(2x, 2y+1) + s(2x+1, 2y+1) + 2) >> 2; W, H: dst size.
__global__ void k_half_u8(const uint8_t *__restrict__ src, size_t sp, int W, int H,
                          uint8_t *__restrict__ dst, size_t dp) {
  const int x = (blockIdx.x * 64 + threadIdx.x) * kStackPx;
  const int y = blockIdx.y * 4 + threadIdx.y;
  if (x >= W || y >= H) return;
  const int n = imin(kStackPx, W - x);
  const uint8_t *r0 = src + (size_t)(2 * y) * sp + 2 * x, *r1 = r0 + sp;
  uint8_t a[16], b[16];
  if (n == kStackPx && ((reinterpret_cast<uintptr_t>(r0) | reinterpret_cast<uintptr_t>(r1)) & 15) == 0) {
    const uint4 t0 = *reinterpret_cast<const uint4 *>(r0), t1 = *reinterpret_cast<const uint4 *>(r1);
    const uint32_t w0[4] = {t0.x, t0.y, t0.z, t0.w}, w1[4] = {t1.x, t1.y, t1.z, t1.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      a[k] = (uint8_t)(w0[k >> 2] >> (8 * (k & 3)));
      b[k] = (uint8_t)(w1[k >> 2] >> (8 * (k & 3)));
    }
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      a[k] = k < 2 * n ? r0[k] : (uint8_t)0;
      b[k] = k < 2 * n ? r1[k] : (uint8_t)0;
    }
  }
  uint32_t out[kStackPx];
#pragma unroll
  for (int j = 0; j < kStackPx; ++j)
    out[j] = ((uint32_t)a[2 * j] + a[2 * j + 1] + b[2 * j] + b[2 * j + 1] + 2u) >> 2;
  store_row8(dst + (size_t)y * dp + x, n, out);
}

struct RemapArgs {
  const uint8_t *frame;
  size_t pitch;          // bytes
  int W, H;              // frame size
  const float *u, *v;
  size_t fpitch;         // floats
  int fw, fh;            // flow size
  double gain;           // 1 / scale: g(t) = float(double(t) * gain)
  double scale_x, scale_y;   // double(fw) / W, double(fh) / H
  int border;
  uint8_t *dst;
  size_t dpitch;         // bytes
  int CW, CH;            // canvas size: W + 2 border, H + 2 border
};

// One canvas row's flow-resize terms (k_resize_hp's bilinear branch, rows)
struct RemapRow {
  int r0, r1;
  float b0, b1;
};

// The flow component at frame px (xc, yc): the plane itself when the sizes agree, else
// cv::resize INTER_LINEAR with half-pixel centres on taps g(.), operation for operation as
// k_resize_hp's bilinear branch (never the 2x area path).
__device__ __forceinline__ float remap_flow_at(const RemapArgs &a, const float *__restrict__ f, int xc,
                                               int yc, const RemapRow &rw, bool same) {
  auto g = [&](float t) { return (float)((double)t * a.gain); };
  if (same) return g(f[(size_t)yc * a.fpitch + xc]);
  float fx = (float)((xc + 0.5) * a.scale_x - 0.5);
  int sx = (int)floorf(fx);
  fx -= (float)sx;
  if (sx < 0) fx = 0.f, sx = 0;
  const bool single = sx + 1 >= a.fw;
  if (sx >= a.fw - 1) fx = 0.f, sx = a.fw - 1;
  const float a0 = 1.f - fx, a1 = fx;
  const float *S0 = f + (size_t)rw.r0 * a.fpitch, *S1 = f + (size_t)rw.r1 * a.fpitch;
  const float t0 = single ? g(S0[sx]) * 1.0f : g(S0[sx]) * a0 + g(S0[sx + 1]) * a1;
  const float t1 = single ? g(S1[sx]) * 1.0f : g(S1[sx]) * a0 + g(S1[sx + 1]) * a1;
  return t0 * rw.b0 + t1 * rw.b1;
}

// Canvas px (X, Y) shows frame coordinate (x, y) = (X - b, Y - b) and takes the flow of the
// nearest frame px; the map (x - U, y - V) is rounded to 1/32 px, the four taps are checked
// against the frame one by one (a tap outside counts 0) and blended with the 5-bit weights.
__global__ void k_remap_flow_u8(RemapArgs a) {
  const int X0 = (blockIdx.x * 64 + threadIdx.x) * kRemapPx;
  const int Y = blockIdx.y * 4 + threadIdx.y;
  if (X0 >= a.CW || Y >= a.CH) return;
  const int n = imin(kRemapPx, a.CW - X0);
  const int y = Y - a.border, yc = imin(imax(y, 0), a.H - 1);
  const bool same = a.fw == a.W && a.fh == a.H;
  RemapRow rw{0, 0, 0.f, 0.f};
  if (!same) {
    float fy = (float)((yc + 0.5) * a.scale_y - 0.5);
    const int sy = (int)floorf(fy);
    fy -= (float)sy;
    rw.b0 = 1.f - fy;
    rw.b1 = fy;
    rw.r0 = imin(imax(sy, 0), a.fh - 1);
    rw.r1 = imin(imax(sy + 1, 0), a.fh - 1);
  }
  uint32_t out[kRemapPx];
#pragma unroll
  for (int j = 0; j < kRemapPx; ++j) {
    out[j] = 0;
    if (j >= n) continue;
    const int x = X0 + j - a.border, xc = imin(imax(x, 0), a.W - 1);
    const float U = remap_flow_at(a, a.u, xc, yc, rw, same);
    const float V = remap_flow_at(a, a.v, xc, yc, rw, same);
    const float mx = (float)x - U, my = (float)y - V;
    const int ix = round_map(mx * 32.f), iy = round_map(my * 32.f);
    const int sx = imin(imax(ix >> 5, -32768), 32767), fx = ix & 31;
    const int sy = imin(imax(iy >> 5, -32768), 32767), fy = iy & 31;
    auto tap = [&](int yy, int xx) -> int {
      if ((unsigned)xx >= (unsigned)a.W || (unsigned)yy >= (unsigned)a.H) return 0;
      return (int)a.frame[(size_t)yy * a.pitch + (size_t)xx];
    };
    const int s00 = tap(sy, sx), s01 = tap(sy, sx + 1), s10 = tap(sy + 1, sx), s11 = tap(sy + 1, sx + 1);
    out[j] = (uint32_t)((s00 * (32 - fx) * (32 - fy) + s01 * fx * (32 - fy) + s10 * (32 - fx) * fy +
                         s11 * fx * fy + 512) >> 10);
  }
  uint8_t *d = a.dst + (size_t)Y * a.dpitch + X0;
  if (n == kRemapPx && (reinterpret_cast<uintptr_t>(d) & 3) == 0) {
    *reinterpret_cast<uint32_t *>(d) = out[0] | out[1] << 8 | out[2] << 16 | out[3] << 24;
  } else {
#pragma unroll
    for (int j = 0; j < kRemapPx; ++j)
      if (j < n) d[j] = (uint8_t)out[j];
  }
}

}  // namespace tvl1k
