// The argument rules of the flow-utility calls (tvl1_fb_score*, tvl1_zero_above*, tvl1_zncc_score*,
// tvl1_warp_by_flow_u8, tvl1_compose_flow*, tvl1_invert_flow*; include/tvl1.h), free of HIP and
// of tvl1_ctx, so that a caller's bad pitch or pair stride never becomes a device access outside
// the memory the caller named.  A call states its planes as a table, its size limit, and which
// planes must not overlap as a table of index pairs; both are walked in order and the first
// fault is the one reported.  Spans are computed with overflow-checked arithmetic: one that does
// not fit the address space is refused, never wrapped into a small one that passes.  Nothing
// here dereferences a plane; tests/test_planes_cpu.py runs it on a CPU under ASan + UBSan.
#pragma once

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/tvl1.h"

namespace tvl1k {

// One plane of each of a call's n pairs: pair b's rows start at p + b * stride + y * pitch
struct Plane {
  const char *name;
  const void *p;
  size_t pitch, stride;   // bytes
  int elem = 4;           // bytes per px: 1 (u8) or 4 (f32)
  bool shared_ok = false; // a pair stride of 0 is one plane shared by every pair
};

// A call's sizes and its plane table.  `skip` is the index of an optional plane the caller left
// out (it is not checked, and no overlap pair that names it is), or -1.
struct PlaneSet {
  int32_t n, w, h;
  const Plane *pl;
  int np, skip;
};

// w and h may not pass 2^log2: `why` says what stops being exact there
struct SizeLimit {
  int log2;
  const char *why;
};
constexpr SizeLimit kFloatXLimit = {24, "float(x) is no longer exact"};
constexpr SizeLimit kMap32Limit = {19, "the 1/32 px map is no longer exact"};

// Planes a and b must not overlap.  An `unless_in_place` pair is waived for a call that runs in
// place (tvl1_compose_flow: c is a exactly), and says so when it is not.
struct Overlap {
  int a, b;
  bool unless_in_place = false;
};

static inline tvl1_status plane_err(std::string *msg, tvl1_status st, const char *fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  *msg = buf;
  return st;
}

// Bytes from a plane's first px to one past its last (h >= 1); false when they do not fit
static inline bool plane_bytes(const Plane &q, int32_t w, int32_t h, size_t *bytes) {
  return !__builtin_mul_overflow(q.pitch, (size_t)(h - 1), bytes) &&
         !__builtin_add_overflow(*bytes, (size_t)w * (size_t)q.elem, bytes);
}

// [lo, hi): the plane's bytes over all n pairs; false when hi does not fit uintptr_t
static inline bool plane_span(const Plane &q, int32_t n, int32_t w, int32_t h, uintptr_t *lo, uintptr_t *hi) {
  size_t pairs, one;
  *lo = reinterpret_cast<uintptr_t>(q.p);
  return !__builtin_mul_overflow((size_t)(n - 1), q.stride, &pairs) && plane_bytes(q, w, h, &one) &&
         !__builtin_add_overflow(pairs, one, &one) && !__builtin_add_overflow(*lo, (uintptr_t)one, hi);
}

// Judged on each plane's whole span over the n pairs.  Spans that do not fit (check_planes
// refuses them) count as overlapping.
static inline bool planes_overlap(const Plane &a, const Plane &b, int32_t n, int32_t w, int32_t h) {
  uintptr_t a0, a1, b0, b1;
  if (!plane_span(a, n, w, h, &a0, &a1) || !plane_span(b, n, w, h, &b0, &b1)) return true;
  return a0 < b1 && b0 < a1;
}

// Everything the calls check about sizes and single planes
static inline tvl1_status check_planes(const PlaneSet &s, const SizeLimit &lim, std::string *msg) {
  const int32_t n = s.n, w = s.w, h = s.h;
  for (int i = 0; i < s.np; ++i)
    if (i != s.skip && !s.pl[i].p) return plane_err(msg, TVL1_EINVAL, "%s is NULL", s.pl[i].name);
  if (n < 1) return plane_err(msg, TVL1_EINVAL, "n must be >= 1 (got %d)", n);
  if (w < 1 || h < 1) return plane_err(msg, TVL1_EINVAL, "bad size %dx%d", w, h);
  if (w > (1 << lim.log2) || h > (1 << lim.log2))
    return plane_err(msg, TVL1_ESIZE, "size %dx%d above 2^%d (%s)", w, h, lim.log2, lim.why);
  for (int i = 0; i < s.np; ++i) {
    const Plane &q = s.pl[i];
    if (i == s.skip) continue;
    if (q.elem == 1) {
      if (q.pitch < (size_t)w) return plane_err(msg, TVL1_EINVAL, "%s: pitch must be >= w", q.name);
    } else {
      if (q.pitch % 4 || q.pitch < (size_t)w * 4)
        return plane_err(msg, TVL1_EINVAL, "%s: pitch must be a multiple of 4 and >= 4 * w", q.name);
      if (q.stride % 4) return plane_err(msg, TVL1_EINVAL, "%s: pair stride must be a multiple of 4", q.name);
    }
    uintptr_t lo, hi;
    size_t one;
    if (!plane_span(q, n, w, h, &lo, &hi) || !plane_bytes(q, w, h, &one))
      return plane_err(msg, TVL1_EINVAL, "%s: plane span overflows the address space", q.name);
    if (n > 1 && !(q.shared_ok && q.stride == 0) && q.stride < one)
      return plane_err(msg, TVL1_EINVAL, "%s: pair stride must cover one plane", q.name);
  }
  return TVL1_OK;
}

// The call's overlap table, in order
static inline tvl1_status check_overlaps(const PlaneSet &s, const Overlap *ov, int nov, bool in_place,
                                         std::string *msg) {
  for (int k = 0; k < nov; ++k) {
    const Plane &a = s.pl[ov[k].a], &b = s.pl[ov[k].b];
    if (ov[k].a == s.skip || ov[k].b == s.skip || (ov[k].unless_in_place && in_place)) continue;
    if (planes_overlap(a, b, s.n, s.w, s.h))
      return plane_err(msg, TVL1_EINVAL, ov[k].unless_in_place ? "%s overlaps %s without being flow a itself"
                                                               : "%s overlaps %s", a.name, b.name);
  }
  return TVL1_OK;
}

}  // namespace tvl1k
