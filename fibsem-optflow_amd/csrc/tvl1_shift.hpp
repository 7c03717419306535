// tvl1_shift.hpp — kernels of the integer drift estimate of a frame pair.
//
// tvl1_estimate_shift finds the integer translation d with I1(x + d) ~= I0(x) between two u8
// frames by a coarse-to-fine search on a 2x2-mean pyramid: every shift of [-R_L, R_L]^2 on the
// coarsest level, then 2 d + {-1, 0, 1}^2 on each finer one.  The cost of a shift is the mean
// absolute difference over the overlap, compared exactly as S_a N_b < S_b N_a in 64-bit
// integers.  Integer arithmetic end to end: tests/shift_ref.py (numpy) and these kernels agree
// in every sum, count and tie.
//
//   k_shift_half    the 2x2 mean (a + b + c + d + 2) >> 2 (k_half_u8's arithmetic) of one frame
//                   of every pair of a batch; the last row / column of an odd level is dropped;
//   k_sad_shifts    S(d) for the (2r + 1)^2 shifts around a base shift, r = 1 .. 4, and on the
//                   finest level S(0, 0) with them, in one pass over the two frames;
//   k_shift_select  one wavefront per pair: the best candidate of a level's table, the next
//                   level's base shift 2 d, and on level 0 the tvl1_shift record.
//
// The planes may be ROI views (any pointer, any pitch): a lane takes 4 adjacent px of a row out
// of the aligned words that lie wholly inside the row, shifted by the address's misalignment,
// and byte by byte where the row's ends leave no such word; no byte outside the row's w px is
// ever touched.  Included by tvl1_engine.hip only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tvl1.h"
#include "tvl1_kernels.hpp"   // imin, imax
#include "tvl1_stack.hpp"     // kStackPx, load_row8, store_row8

namespace tvl1k {

constexpr int kShiftMaxR = 4;                  // radius of one table
constexpr int kShiftZeroSlot = 81;             // S(0, 0) of level 0, after the 9 x 9 table
constexpr int kShiftSlots = 82;                // u64 slots per pair and level
constexpr int kShiftBand = 256;                // px of a row per wavefront: 64 lanes x 4 px

// One frame of every pair, one pyramid step.  Grid (x blocks, pair, row blocks); W, H: dst size.
__global__ void k_shift_half(const uint8_t *__restrict__ src, size_t sp, size_t sstride, int W, int H,
                             uint8_t *__restrict__ dst, size_t dp, size_t dstride) {
  const int pair = __builtin_amdgcn_readfirstlane(blockIdx.y);
  const int x = (blockIdx.x * 64 + threadIdx.x) * kStackPx;
  const int y = blockIdx.z * 4 + threadIdx.y;
  if (x >= W || y >= H) return;
  const int n = imin(kStackPx, W - x);
  const uint8_t *r0 = src + (size_t)pair * sstride + (size_t)(2 * y) * sp + 2 * x, *r1 = r0 + sp;
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
  store_row8(dst + (size_t)pair * dstride + (size_t)y * dp + x, n, out);
}

// The 4 px at columns x .. x + 3 of a row of w px, px i in byte i, byte by byte; columns outside
// [0, w) read 0 and are never touched.
__device__ __forceinline__ uint32_t shift_load4_bytes(const uint8_t *row, int x, int w) {
  uint32_t v = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (x + i >= 0 && x + i < w) v |= (uint32_t)row[x + i] << (8 * i);
  return v;
}

// K words of a row of w px, word k = the px at columns x + 4k .. x + 4k + 3 with x = xu + xl, xu
// wavefront-uniform and xl a multiple of 4 (the lane's part), so the misalignment m of the
// address row + x is uniform.  A lane whose 4K px all lie in aligned words wholly inside the row
// reads K + 1 of those (K when m = 0): straight-line loads, nothing outside the row's w px
// touched; shift_words_get shifts them by m bytes where the words are used, so a step's loads
// are in flight together.  The other lanes (the row's first and last px at most, and every lane
// of a row too narrow to hold K + 1 aligned words) go byte by byte, reading 0 outside.
template <int K>
struct ShiftWords {
  uint32_t t[K + 1];   // aligned words (fast lanes)
  uint32_t q[K];       // the words themselves (the other lanes)
  uint32_t m;
  bool fast;
};

template <int K>
__device__ __forceinline__ ShiftWords<K> shift_words_load(const uint8_t *row, int xu, int xl, int w) {
  ShiftWords<K> s;
  const int r3 = (int)(reinterpret_cast<uintptr_t>(row) & 3);
  const int lo = (4 - r3) & 3, hi = ((r3 + w) & ~3) - 4 - r3;   // columns of the first and last such word
  const int m = (r3 + xu) & 3;
  const int n = m ? K + 1 : K;
  const int top = hi - 4 * (n - 1);   // the last column at which n words still fit
  const int x = xu + xl, xa = x - m;
  s.m = (uint32_t)m;
  s.fast = false;
#pragma unroll
  for (int k = 0; k < K; ++k) s.t[k] = 0, s.q[k] = 0;
  s.t[K] = 0;
  if (top >= lo) {   // uniform
    s.fast = xa >= lo && xa <= top;
    const int c = imin(imax(xa, lo), top);
#pragma unroll
    for (int k = 0; k < K; ++k) s.t[k] = *reinterpret_cast<const uint32_t *>(row + c + 4 * k);
    s.t[K] = *reinterpret_cast<const uint32_t *>(row + imin(c + 4 * K, hi));   // unused when m = 0
  }
  if (!s.fast) {
#pragma unroll
    for (int k = 0; k < K; ++k) s.q[k] = shift_load4_bytes(row, x + 4 * k, w);
  }
  return s;
}

template <int K>
__device__ __forceinline__ uint32_t shift_words_get(const ShiftWords<K> &s, int k) {
  return s.fast ? __builtin_amdgcn_alignbyte(s.t[k + 1], s.t[k], s.m) : s.q[k];
}

// 0xff in byte i where I0 column x + i and I1 column x + i + dx both lie in [0, w)
__device__ __forceinline__ uint32_t shift_colmask(int x, int dx, int w) {
  uint32_t m = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (x + i < w && x + i + dx >= 0 && x + i + dx < w) m |= 0xffu << (8 * i);
  return m;
}

struct ShiftSadArgs {
  const uint8_t *I0, *I1;
  size_t p0, p1;          // row pitch (bytes)
  size_t s0, s1;          // pair stride (bytes; 0: one frame for every pair)
  int w, h;
  const int2 *base;       // per pair: the table's centre shift; NULL: (cx, cy) for every pair
  int cx, cy;
  int seg;                // I0 rows per wavefront
  unsigned long long *table;   // kShiftSlots per pair, zero before the launch
};

// S(c + (dx, dy)) for dx, dy in [-R, R], slot (dy + R) (2R + 1) + (dx + R); ZERO: S(0, 0) too,
// slot kShiftZeroSlot.  Grid (256-px bands, pair, groups of 4 row segments); a wavefront walks
// down the I0 rows of its segment of one band.  Each I1 row it meets is loaded once as the
// three words around column x + cx, turned into the 2R + 1 dx-shifted words by byte alignment
// of neighbouring words, masked to the overlap's columns and kept in a ring of 2R + 1 rows, so
// it serves every dy; an I0 word, masked the same way, then meets the whole ring with one
// packed byte SAD per shift.  Masked px are 0 on both sides and add 0; rows outside the
// overlap are skipped (a wavefront-uniform branch).  Per-lane u32 partials: at most 1020 a
// word and seg words, so even a wavefront's sum stays below 2^23; they widen to u64 where the
// block adds its sums to the table (integer atomics: any order gives the same table).
template <int R, bool ZERO>
__global__ __launch_bounds__(256) void k_sad_shifts(ShiftSadArgs a) {
  constexpr int D = 2 * R + 1;
  const int pair = __builtin_amdgcn_readfirstlane(blockIdx.y);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
  int cx = a.cx, cy = a.cy;
  if (a.base) {
    const int2 b = a.base[pair];
    cx = __builtin_amdgcn_readfirstlane(b.x);
    cy = __builtin_amdgcn_readfirstlane(b.y);
  }
  const uint8_t *I0 = a.I0 + (size_t)pair * a.s0, *I1 = a.I1 + (size_t)pair * a.s1;
  const int w = a.w, h = a.h;
  const int xb = blockIdx.x * kShiftBand, xl = threadIdx.x * 4, x0 = xb + xl;
  const int y0 = __builtin_amdgcn_readfirstlane((blockIdx.z * 4 + wv) * a.seg);
  const int y1 = imin(y0 + a.seg, h);

  uint32_t m[D], ring[D][D], acc[D][D], accz = 0;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    m[i] = shift_colmask(x0, cx + i - R, w);
#pragma unroll
    for (int k = 0; k < D; ++k) ring[k][i] = 0, acc[k][i] = 0;
  }
  uint32_t valid = 0;   // bit k: ring row k holds an I1 row of the frame
  // step j brings I1 row j into the ring's last row; the ring then holds rows j - 2R .. j, all
  // that I0 row j - cy - R needs.  A step's loads are all issued before the first of them is used.
  struct Step {
    ShiftWords<3> i1;
    ShiftWords<1> p, z;
  };
  auto load = [&](int j) {
    Step s{};
    if (j >= 0 && j < h) s.i1 = shift_words_load<3>(I1 + (size_t)j * a.p1, xb + cx - 4, xl, w);
    const int y = j - cy - R;
    if (y >= y0 && y < y1) {
      s.p = shift_words_load<1>(I0 + (size_t)y * a.p0, xb, xl, w);
      if (ZERO) s.z = shift_words_load<1>(I1 + (size_t)y * a.p1, xb, xl, w);
    }
    return s;
  };
  for (int j = y0 + cy - R; j < y1 + cy + R; ++j) {
    const Step cur = load(j);
#pragma unroll
    for (int k = 0; k + 1 < D; ++k)
#pragma unroll
      for (int i = 0; i < D; ++i) ring[k][i] = ring[k + 1][i];
    valid >>= 1;
    if (j >= 0 && j < h) {
      const uint32_t w0 = shift_words_get(cur.i1, 0), w1 = shift_words_get(cur.i1, 1),
                     w2 = shift_words_get(cur.i1, 2);
#pragma unroll
      for (int i = 0; i < D; ++i) {
        const int dx = i - R;   // the word at column x0 + cx + dx
        const uint32_t s = dx == -4  ? w0
                           : dx < 0  ? __builtin_amdgcn_alignbyte(w1, w0, (uint32_t)(4 + dx))
                           : dx == 0 ? w1
                           : dx < 4  ? __builtin_amdgcn_alignbyte(w2, w1, (uint32_t)dx)
                                     : w2;
        ring[D - 1][i] = s & m[i];
      }
      valid |= 1u << (D - 1);
    }
    const int y = j - cy - R;
    if (y >= y0 && y < y1) {
      const uint32_t p = shift_words_get(cur.p, 0);
      uint32_t pm[D];
#pragma unroll
      for (int i = 0; i < D; ++i) pm[i] = p & m[i];
#pragma unroll
      for (int k = 0; k < D; ++k)
        if (valid >> k & 1u) {
#pragma unroll
          for (int i = 0; i < D; ++i) acc[k][i] = __builtin_amdgcn_sad_u8(pm[i], ring[k][i], acc[k][i]);
        }
      if (ZERO) accz = __builtin_amdgcn_sad_u8(p, shift_words_get(cur.z, 0), accz);   // both read 0 outside the row
    }
  }

  __shared__ uint32_t red[4][kShiftSlots];
#pragma unroll
  for (int k = 0; k < D; ++k)
#pragma unroll
    for (int i = 0; i < D; ++i) {
      uint32_t v = acc[k][i];
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
      if (threadIdx.x == 0) red[wv][k * D + i] = v;
    }
  if (ZERO) {
    for (int o = 32; o > 0; o >>= 1) accz += __shfl_xor(accz, o);
    if (threadIdx.x == 0) red[wv][kShiftZeroSlot] = accz;
  }
  __syncthreads();
  const int t = threadIdx.y * 64 + threadIdx.x;
  const int slot = t < D * D ? t : (ZERO && t == D * D ? kShiftZeroSlot : -1);
  if (slot >= 0) {
    const unsigned long long s = (unsigned long long)red[0][slot] + red[1][slot] + red[2][slot] + red[3][slot];
    if (s) atomicAdd(a.table + (size_t)pair * kShiftSlots + slot, s);
  }
}

struct ShiftCand {
  unsigned long long S, N;
  int dx, dy, has;
};

// a better than b: the smaller mean S / N, compared exactly as S_a N_b < S_b N_a (S < 2^34,
// N <= 2^26); then the smaller dx^2 + dy^2, then dy, then dx.  A total order on distinct shifts.
__device__ __forceinline__ bool shift_better(const ShiftCand &a, const ShiftCand &b) {
  if (!a.has || !b.has) return a.has && !b.has;
  const unsigned long long l = a.S * b.N, r = b.S * a.N;
  if (l != r) return l < r;
  const int na = a.dx * a.dx + a.dy * a.dy, nb = b.dx * b.dx + b.dy * b.dy;
  if (na != nb) return na < nb;
  if (a.dy != b.dy) return a.dy < b.dy;
  return a.dx < b.dx;
}

struct ShiftSelArgs {
  const unsigned long long *table;   // kShiftSlots per pair
  const int2 *base;                  // the table's centre per pair; NULL: (0, 0)
  int w, h;                          // the level's size
  int r;                             // the table's radius
  int Rl;                            // largest |dx|, |dy| of a candidate on this level
  int last;                          // level 0: (0, 0) is a candidate too, and out is written
  int levels;
  int2 *next;                        // per pair: 2 d, the next finer level's centre (or NULL)
  tvl1_shift *out;                   // per pair (level 0)
};

// Grid (1, pairs), one wavefront each.
__global__ __launch_bounds__(64) void k_shift_select(ShiftSelArgs a) {
  const int pair = __builtin_amdgcn_readfirstlane(blockIdx.y);
  const unsigned long long *T = a.table + (size_t)pair * kShiftSlots;
  int bx = 0, by = 0;
  if (a.base) {
    const int2 b = a.base[pair];
    bx = __builtin_amdgcn_readfirstlane(b.x);
    by = __builtin_amdgcn_readfirstlane(b.y);
  }
  const int D = 2 * a.r + 1;
  ShiftCand best{0, 1, 0, 0, 0};
  for (int t = threadIdx.x; t < D * D + (a.last ? 1 : 0); t += 64) {
    ShiftCand c;
    if (t < D * D) {
      c.dx = bx + t % D - a.r;
      c.dy = by + t / D - a.r;
      c.S = T[t];
    } else {
      c.dx = c.dy = 0;
      c.S = T[kShiftZeroSlot];
    }
    const int ow = a.w - abs(c.dx), oh = a.h - abs(c.dy);
    c.has = abs(c.dx) <= a.Rl && abs(c.dy) <= a.Rl && ow > 0 && oh > 0;
    c.N = c.has ? (unsigned long long)ow * (unsigned long long)oh : 1ull;
    if (shift_better(c, best)) best = c;
  }
  for (int o = 32; o > 0; o >>= 1) {
    ShiftCand c;
    c.S = __shfl_xor(best.S, o);
    c.N = __shfl_xor(best.N, o);
    c.dx = __shfl_xor(best.dx, o);
    c.dy = __shfl_xor(best.dy, o);
    c.has = __shfl_xor(best.has, o);
    if (shift_better(c, best)) best = c;
  }
  if (threadIdx.x != 0) return;
  if (a.next) a.next[pair] = make_int2(2 * best.dx, 2 * best.dy);
  if (a.last) {
    tvl1_shift o;
    o.dx = best.dx, o.dy = best.dy, o.levels = a.levels, o.reserved = 0;
    o.sad = best.S, o.count = best.N;
    o.sad_zero = T[kShiftZeroSlot];
    o.count_zero = (unsigned long long)a.w * (unsigned long long)a.h;
    a.out[pair] = o;
  }
}

// The hand-over to a seeded batch (tvl1_calc_batch_auto_init): the level-0 records of n pairs
// as kb_flow_down_const's per-pair constants, seed[2 b] = (float)dx_b, seed[2 b + 1] =
// (float)dy_b, read where k_shift_select left them (no host read between estimate and solve).
__global__ void k_shift_seed(const tvl1_shift *__restrict__ recs, int n, float *__restrict__ seed) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= n) return;
  seed[2 * b] = (float)recs[b].dx;
  seed[2 * b + 1] = (float)recs[b].dy;
}

}  // namespace tvl1k
