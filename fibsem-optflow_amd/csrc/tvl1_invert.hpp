// tvl1_invert.hpp — the kernel of flow inversion.
//
// Given the flow f = (uf, vf) of a pair A -> B, the flow g of B -> A on B's grid is the fixed point
// of
//
//   g(y) = -f(y + g(y))
//
// started at g0 = -f(y) and iterated K times; one more sample at g_K gives the residual
// |g_K + f(y + g_K)|^2 and whether the last landing lies inside the frame.  A px's iteration reads
// its own g_k and the immutable f only, so all K + 1 samples of a px run in registers in one launch.
// A landing point outside the frame is clamped to it exactly as k_compose_flow clamps (NaN and
// -inf to 0, +inf to the far edge), so no tap is ever read outside the plane whatever the input; a
// NaN or an infinity in f propagates into g and never becomes an address.  Every float operation
// is one IEEE f32 rounding in the order of tests/invert_ref.py (numpy), whatever the ctx's
// fast_math or profile: contraction is switched off in the functions themselves.
//
// Two arms, one template: k_invert_flow<false> gathers every tap from global memory;
// k_invert_flow<true> first stages in LDS the box of f that the block's px land on (placed by the
// flow itself: chains are 20-30 px long, so a window centred on the tile would not cover them),
// and a px whose taps leave the box in some iteration gathers that iteration from global memory.
// Both arms blend the taps with inv_blend, so their bits cannot differ.
//
// The planes may be ROI views, with k_fb_score's ownership: a lane owns 4 adjacent px of a row
// and moves them as one 16-byte word where the row address allows, float by float otherwise; no
// float outside a row's w px is ever touched.  Nothing runs in place: a px reads f at other px.
// Included by tvl1_engine.hip only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tvl1_fbcheck.hpp"   // kFbPx, fb_load4, fb_store4

namespace tvl1k {

// The window arm's geometry (parsed by tests/invert_cases.py: keep one constant per line)
constexpr int kInvTileW = 256;       // px of a row per block: 64 lanes x kFbPx
constexpr int kInvTileH = 4;         // rows per block and row step: one per wavefront
constexpr int kInvDrift = 3;         // px the box is grown by on every side for later iterations
constexpr int kInvWinFloats = 4000;  // floats of one plane's window: 2 x 16000 B of LDS per block
constexpr int kInvMaxIter = 32;

struct InvertArgs {
  const float *uf, *vf;
  size_t fp, fs;          // flow A -> B: row pitch and pair stride (bytes)
  float *ug, *vg;
  size_t gp, gs;          // flow B -> A
  float *resid;           // or NULL
  size_t rp, rs;
  int w, h;
  int iters;              // K: 1..kInvMaxIter
  float tol;
  unsigned long long *count;   // per pair {outside, unconverged}, zero before the launch; or NULL
};

struct InvTap {
  int x0, x1, y0, y1;
  float ax, ay;
  bool inside;
};

// Where px (x, y) lands by g, clamped to the frame: the conversions are in range for any g
__device__ __forceinline__ InvTap inv_land(int x, int y, float gu, float gv, int w, int h, float xmax,
                                           float ymax) {
#pragma clang fp contract(off)
  InvTap t;
  const float X = (float)x + gu;
  const float Y = (float)y + gv;
  t.inside = X >= 0.0f && X <= xmax && Y >= 0.0f && Y <= ymax;   // false for NaN
  const float Xc = X >= 0.0f ? (X <= xmax ? X : xmax) : 0.0f;
  const float Yc = Y >= 0.0f ? (Y <= ymax ? Y : ymax) : 0.0f;
  const float fx = floorf(Xc), fy = floorf(Yc);
  t.x0 = (int)fx, t.y0 = (int)fy;
  t.ax = Xc - fx, t.ay = Yc - fy;
  t.x1 = imin(t.x0 + 1, w - 1), t.y1 = imin(t.y0 + 1, h - 1);
  return t;
}

// fb_sample's arithmetic on four taps that are already in registers
__device__ __forceinline__ float inv_blend(float p00, float p01, float p10, float p11, float ax, float ay) {
#pragma clang fp contract(off)
  const float t = p00 + ax * (p01 - p00);
  const float b = p10 + ax * (p11 - p10);
  return t + ay * (b - t);
}

// The block's window: rows by0..by1, columns bx0..bx1 of both planes, bw floats a row
struct InvBox {
  bool on;
  int bx0, bx1, by0, by1, bw;
  const float *wu, *wv;
};

// One sample of f at y + g for the m px of a lane: the taps of all px are fetched before any is
// blended, so the gathers of an iteration are in flight together
template <bool kWin>
__device__ __forceinline__ void inv_step(const char *uf, const char *vf, size_t fp, int w, int h, float xmax,
                                         float ymax, int x, int y, int m, const InvBox &bx,
                                         const float gu[kFbPx], const float gv[kFbPx], float us[kFbPx],
                                         float vs[kFbPx], bool inside[kFbPx]) {
#pragma clang fp contract(off)
  InvTap t[kFbPx];
  float pu[kFbPx][4], pv[kFbPx][4];
#pragma unroll
  for (int k = 0; k < kFbPx; ++k) {
    t[k] = inv_land(x + k, y, gu[k], gv[k], w, h, xmax, ymax);
    inside[k] = t[k].inside;
#pragma unroll
    for (int j = 0; j < 4; ++j) pu[k][j] = pv[k][j] = 0.0f;
    if (k >= m) continue;
    if (kWin && bx.on && t[k].x0 >= bx.bx0 && t[k].x1 <= bx.bx1 && t[k].y0 >= bx.by0 && t[k].y1 <= bx.by1) {
      const int i0 = (t[k].y0 - bx.by0) * bx.bw + (t[k].x0 - bx.bx0);
      const int dx = t[k].x1 - t[k].x0, dy = (t[k].y1 - t[k].y0) * bx.bw;
      pu[k][0] = bx.wu[i0], pu[k][1] = bx.wu[i0 + dx], pu[k][2] = bx.wu[i0 + dy], pu[k][3] = bx.wu[i0 + dy + dx];
      pv[k][0] = bx.wv[i0], pv[k][1] = bx.wv[i0 + dx], pv[k][2] = bx.wv[i0 + dy], pv[k][3] = bx.wv[i0 + dy + dx];
    } else {
      const size_t o0 = (size_t)t[k].y0 * fp, o1 = (size_t)t[k].y1 * fp;
      const float *u0 = reinterpret_cast<const float *>(uf + o0), *u1 = reinterpret_cast<const float *>(uf + o1);
      const float *v0 = reinterpret_cast<const float *>(vf + o0), *v1 = reinterpret_cast<const float *>(vf + o1);
      pu[k][0] = u0[t[k].x0], pu[k][1] = u0[t[k].x1], pu[k][2] = u1[t[k].x0], pu[k][3] = u1[t[k].x1];
      pv[k][0] = v0[t[k].x0], pv[k][1] = v0[t[k].x1], pv[k][2] = v1[t[k].x0], pv[k][3] = v1[t[k].x1];
    }
  }
#pragma unroll
  for (int k = 0; k < kFbPx; ++k) {
    us[k] = inv_blend(pu[k][0], pu[k][1], pu[k][2], pu[k][3], t[k].ax, t[k].ay);
    vs[k] = inv_blend(pv[k][0], pv[k][1], pv[k][2], pv[k][3], t[k].ax, t[k].ay);
  }
}

// Grid and ownership as k_compose_flow's: (256-px tiles, pair, row groups), block 64 x 4, rows
// walked 4 gridDim.z apart; the row step is uniform over the block (the window arm meets at
// barriers inside it).  A lane whose px have all reached a fixed point bit for bit (g_{k+1} ==
// g_k: every later step reproduces it, and the sample just taken is the last one's) leaves the
// iteration.  Counts per pair {outside, unconverged}: k_zero_above's pattern.
template <bool kWin>
__global__ __launch_bounds__(256) void k_invert_flow(InvertArgs a) {
#pragma clang fp contract(off)
  const int pair = __builtin_amdgcn_readfirstlane(blockIdx.y);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
  const int x = (blockIdx.x * 64 + threadIdx.x) * kFbPx;
  const int n = imax(0, imin(kFbPx, a.w - x));
  const char *uf = reinterpret_cast<const char *>(a.uf) + (size_t)pair * a.fs;
  const char *vf = reinterpret_cast<const char *>(a.vf) + (size_t)pair * a.fs;
  char *ug = reinterpret_cast<char *>(a.ug) + (size_t)pair * a.gs;
  char *vg = reinterpret_cast<char *>(a.vg) + (size_t)pair * a.gs;
  char *rs = a.resid ? reinterpret_cast<char *>(a.resid) + (size_t)pair * a.rs : nullptr;
  const float xmax = (float)(a.w - 1), ymax = (float)(a.h - 1);
  const int ystep = (int)gridDim.z * kInvTileH;
  __shared__ float win_u[kWin ? kInvWinFloats : 1], win_v[kWin ? kInvWinFloats : 1];
  __shared__ int ext[kInvTileH][4];
  uint32_t c_out = 0, c_unc = 0;
  for (int yb = blockIdx.z * kInvTileH; yb < a.h; yb += ystep) {   // block-uniform
    const int y = yb + wv;
    const int m = y < a.h ? n : 0;   // this lane's px of this row step
    float u[kFbPx], v[kFbPx], gu[kFbPx], gv[kFbPx];
#pragma unroll
    for (int k = 0; k < kFbPx; ++k) u[k] = v[k] = 0.0f;
    if (m > 0) {
      fb_load4(reinterpret_cast<const float *>(uf + (size_t)y * a.fp) + x, m, u);
      fb_load4(reinterpret_cast<const float *>(vf + (size_t)y * a.fp) + x, m, v);
    }
#pragma unroll
    for (int k = 0; k < kFbPx; ++k) gu[k] = -u[k], gv[k] = -v[k];
    InvBox bx;
    bx.on = false, bx.bx0 = bx.bx1 = bx.by0 = bx.by1 = bx.bw = 0, bx.wu = win_u, bx.wv = win_v;
    if (kWin) {
      // the bounding box of the block's first landings: lanes, a wavefront, four wavefronts
      int lx0 = 0x7fffffff, ly0 = 0x7fffffff, lx1 = -1, ly1 = -1;
#pragma unroll
      for (int k = 0; k < kFbPx; ++k) {
        if (k >= m) continue;
        const InvTap t = inv_land(x + k, y, gu[k], gv[k], a.w, a.h, xmax, ymax);
        lx0 = imin(lx0, t.x0), lx1 = imax(lx1, t.x0), ly0 = imin(ly0, t.y0), ly1 = imax(ly1, t.y0);
      }
      for (int o = 32; o > 0; o >>= 1) {
        lx0 = imin(lx0, __shfl_xor(lx0, o)), ly0 = imin(ly0, __shfl_xor(ly0, o));
        lx1 = imax(lx1, __shfl_xor(lx1, o)), ly1 = imax(ly1, __shfl_xor(ly1, o));
      }
      if (threadIdx.x == 0) ext[wv][0] = lx0, ext[wv][1] = lx1, ext[wv][2] = ly0, ext[wv][3] = ly1;
      __syncthreads();
#pragma unroll
      for (int r = 0; r < kInvTileH; ++r) {
        lx0 = imin(lx0, ext[r][0]), lx1 = imax(lx1, ext[r][1]);
        ly0 = imin(ly0, ext[r][2]), ly1 = imax(ly1, ext[r][3]);
      }
      lx0 = __builtin_amdgcn_readfirstlane(lx0), lx1 = __builtin_amdgcn_readfirstlane(lx1);
      ly0 = __builtin_amdgcn_readfirstlane(ly0), ly1 = __builtin_amdgcn_readfirstlane(ly1);
      if (lx1 >= 0) {   // the block has a px in this row step
        // the drift of later iterations on every side, and the bilinear tap on the far one
        bx.bx0 = imax(lx0 - kInvDrift, 0), bx.bx1 = imin(lx1 + kInvDrift + 1, a.w - 1);
        bx.by0 = imax(ly0 - kInvDrift, 0), bx.by1 = imin(ly1 + kInvDrift + 1, a.h - 1);
        bx.bw = bx.bx1 - bx.bx0 + 1;
        const int bh = bx.by1 - bx.by0 + 1;
        bx.on = (long long)bx.bw * bh <= kInvWinFloats;   // block-uniform
        if (bx.on) {
          for (int r = wv; r < bh; r += kInvTileH) {
            const size_t o = (size_t)(bx.by0 + r) * a.fp;
            const float *ru = reinterpret_cast<const float *>(uf + o) + bx.bx0;
            const float *rv = reinterpret_cast<const float *>(vf + o) + bx.bx0;
            for (int c = threadIdx.x; c < bx.bw; c += 64)
              win_u[r * bx.bw + c] = ru[c], win_v[r * bx.bw + c] = rv[c];
          }
        }
      }
      __syncthreads();
    }
    if (m > 0) {
      float us[kFbPx], vs[kFbPx];
      bool in[kFbPx];
      for (int it = 0;; ++it) {
        inv_step<kWin>(uf, vf, a.fp, a.w, a.h, xmax, ymax, x, y, m, bx, gu, gv, us, vs, in);
        if (it == a.iters) break;
        bool fixed = true;
#pragma unroll
        for (int k = 0; k < kFbPx; ++k) {
          const float nu = -us[k], nv = -vs[k];
          fixed &= k >= m || (__float_as_uint(nu) == __float_as_uint(gu[k]) &&
                              __float_as_uint(nv) == __float_as_uint(gv[k]));
          gu[k] = nu, gv[k] = nv;
        }
        if (fixed) break;
      }
      float res[kFbPx];
#pragma unroll
      for (int k = 0; k < kFbPx; ++k) {
        const float ex = gu[k] + us[k], ey = gv[k] + vs[k];
        res[k] = ex * ex + ey * ey;
        if (k < m) {
          c_out += in[k] ? 0u : 1u;
          c_unc += res[k] <= a.tol ? 0u : 1u;   // NaN is unconverged
        }
      }
      fb_store4(reinterpret_cast<float *>(ug + (size_t)y * a.gp) + x, m, gu);
      fb_store4(reinterpret_cast<float *>(vg + (size_t)y * a.gp) + x, m, gv);
      if (rs) fb_store4(reinterpret_cast<float *>(rs + (size_t)y * a.rp) + x, m, res);
    }
    if (kWin) __syncthreads();   // the next row step rewrites the window and ext
  }
  if (!a.count) return;   // a kernel argument: the whole block leaves
  for (int o = 32; o > 0; o >>= 1) c_out += __shfl_xor(c_out, o), c_unc += __shfl_xor(c_unc, o);
  __shared__ uint32_t red[kInvTileH][2];
  if (threadIdx.x == 0) red[wv][0] = c_out, red[wv][1] = c_unc;
  __syncthreads();
  if (threadIdx.x == 0 && threadIdx.y == 0) {
    const unsigned long long t0 = (unsigned long long)red[0][0] + red[1][0] + red[2][0] + red[3][0];
    const unsigned long long t1 = (unsigned long long)red[0][1] + red[1][1] + red[2][1] + red[3][1];
    if (t0) atomicAdd(a.count + 2 * (size_t)pair, t0);
    if (t1) atomicAdd(a.count + 2 * (size_t)pair + 1, t1);
  }
}

}  // namespace tvl1k
