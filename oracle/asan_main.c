/* TEST INFRASTRUCTURE: drives the oracle under ASan + UBSan (`make -C oracle asan`,
 * tests/test_oracle_cpu.py::test_oracle_under_asan_ubsan).  Solves small synthetic pairs
 * at odd sizes through every code path of the restatement: both profiles, gamma, median,
 * fixed work, a pyramid that bottoms out, 1x1 / 16x16 edge sizes, and the seeded entry in
 * both arithmetics (a pitched seed whose taps leave the frame on every side); the fast branch
 * (orc_set_approx_prims with C stand-ins: 1.0f / x and sqrtf) at every size, 1x1 included,
 * unseeded, seeded and from f32 frames, with a failing primitive, and uninstalled again; and the
 * pre-alignment restatement (tvl1_oracle_align.c) at its edges: frames with one candidate
 * px and with none, a pitched view, a level quota sum above nfeatures, train sets of 0, 1
 * and 65 descriptors, singular and far-off warps, and a pair of different sizes; and profile 1
 * on its own edges (tests/dualtvl1_cases.py): scale_step 0.5 on sizes whose levels round up
 * (35 -> 18: the 2x area path at the border of an odd source), and frames smaller than the
 * bicubic remap's 4 x 4 taps and the median's window. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <math.h>

#include "tvl1_oracle.h"

/* stand-ins for the fast branch's primitives; g_prim_calls counts them, g_prim_fail makes the
 * call of that number fail */
static int g_prim_calls = 0, g_prim_fail = -1;
static int rcp_c(const float *in, float *out, size_t n) {
  if (g_prim_calls++ == g_prim_fail) return 1;
  for (size_t i = 0; i < n; ++i) out[i] = 1.0f / in[i];
  return 0;
}
static int sqrt_c(const float *in, float *out, size_t n) {
  if (g_prim_calls++ == g_prim_fail) return 1;
  for (size_t i = 0; i < n; ++i) out[i] = sqrtf(in[i]);
  return 0;
}

static void pair(int w, int h, unsigned seed, uint8_t *a, uint8_t *b) {
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      seed = seed * 1103515245u + 12345u;
      const int v = 40 + (int)((seed >> 16) % 160);
      a[y * w + x] = (uint8_t)v;
      b[y * w + (x + 1) % w] = (uint8_t)(v + ((seed >> 8) & 3));
    }
}

/* a frame with corners everywhere: uniform noise from the same generator */
static void noise(int w, int h, size_t pitch, unsigned seed, uint8_t *a) {
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      seed = seed * 1103515245u + 12345u;
      a[(size_t)y * pitch + x] = (uint8_t)(seed >> 16);
    }
}

static const tvl1_align_params kOrb = {5000, 1.2f, 8, 16, 0, 2, 31, 20, 0, 0.8f, 8, 5.0};

/* orc_orb_detect into outputs of exactly cap rows; returns the count */
static int detect(const uint8_t *img, size_t pitch, int w, int h, const tvl1_align_params *ap, int cap,
                  uint8_t **desc_out) {
  float *kp = malloc(sizeof(float) * 5 * (size_t)(cap > 0 ? cap : 1));
  uint8_t *desc = malloc(32 * (size_t)(cap > 0 ? cap : 1));
  const int n = orc_orb_detect(img, pitch, w, h, ap, kp, desc, cap);
  free(kp);
  if (desc_out)
    *desc_out = desc;
  else
    free(desc);
  return n;
}

static int align_paths(void) {
  int fails = 0;
  /* one candidate px, none, tile seams; a pitched view equals its packed copy */
  static const int sizes[][2] = {{33, 33}, {32, 40}, {129, 97}};
  for (size_t si = 0; si < sizeof sizes / sizeof sizes[0]; ++si) {
    const int w = sizes[si][0], h = sizes[si][1];
    const size_t pitch = (size_t)w + 71;
    uint8_t *packed = malloc((size_t)w * h), *parent = malloc(pitch * (h + 8));
    noise(w, h, (size_t)w, 3u + (unsigned)si, packed);
    memset(parent, 0x55, pitch * (h + 8));
    for (int y = 0; y < h; ++y) memcpy(parent + (size_t)(y + 5) * pitch + 3, packed + (size_t)y * w, w);
    uint8_t *d0 = NULL, *d1 = NULL;
    const int n0 = detect(packed, (size_t)w, w, h, &kOrb, 4096, &d0);
    const int n1 = detect(parent + 5 * pitch + 3, pitch, w, h, &kOrb, 4096, &d1);
    const int nshort = detect(packed, (size_t)w, w, h, &kOrb, n0 > 10 ? n0 - 10 : 0, NULL);
    if (n0 < 0 || n0 != n1 || nshort != n0 || memcmp(d0, d1, 32 * (size_t)(n0 < 4096 ? n0 : 4096)) != 0 ||
        (w == 32 && n0 != 0) || (w == 129 && n0 < 100)) {
      fprintf(stderr, "orb %dx%d: %d packed, %d pitched, %d short\n", w, h, n0, n1, nshort);
      ++fails;
    }
    /* the match list over train sets of 0, 1 and 65 descriptors */
    if (w == 129) {
      static const int nts[] = {0, 1, 65};
      for (size_t k = 0; k < sizeof nts / sizeof nts[0]; ++k) {
        const int nq = 3, nt = nts[k];
        int32_t idx[6], dist[6];
        orc_match_knn2(d0, nq, d0, nt, idx, dist);
        const int want1 = nt > 1 ? 1 : 0;
        for (int i = 0; i < nq; ++i)
          if ((nt > i && (idx[2 * i] != i || dist[2 * i] != 0)) || (nt == 0 && idx[2 * i] != -1) ||
              (idx[2 * i + 1] >= 0) != want1) {
            fprintf(stderr, "match nt %d query %d: %d %d\n", nt, i, idx[2 * i], idx[2 * i + 1]);
            ++fails;
          }
      }
    }
    free(d0);
    free(d1);
    free(packed);
    free(parent);
  }
  /* 16 levels at 1.1 with 16 features: the level quotas add up to 17 */
  {
    const int w = 400, h = 300;
    uint8_t *a = malloc((size_t)w * h);
    noise(w, h, (size_t)w, 11u, a);
    tvl1_align_params ap = kOrb;
    ap.nlevels = 16, ap.scale_factor = 1.1f, ap.nfeatures = 16;
    const int n = detect(a, (size_t)w, w, h, &ap, 17, NULL);
    float aff[6];
    int ng = -1, oc = -1;
    const int rc = orc_find_alignment(a, (size_t)w, w, h, a, (size_t)w, w, h, &ap, aff, &ng, &oc);
    if (n != 17 || rc != 0 || ng != 16) {
      fprintf(stderr, "budget: %d keypoints, status %d, %d good, outcome %d\n", n, rc, ng, oc);
      ++fails;
    }
    free(a);
  }
  /* singular (every px samples src(0, 0)) and far-off (all zero) warps, pitched planes */
  {
    enum { SW = 33, SH = 9, SP = 40, DW = 65, DH = 5, DP = 70 };
    uint8_t src[SH * SP], dst[DH * DP];
    noise(SW, SH, SP, 5u, src);
    static const float Ms[3][6] = {{1, 2, 3, 2, 4, -1}, {1, 0, 1e6f, 0, 1, 1e6f}, {1, 0, -1e6f, 0, 1, -1e6f}};
    for (int k = 0; k < 3; ++k) {
      memset(dst, 0xA5, sizeof dst);
      orc_warp_affine_u8(src, SP, SW, SH, dst, DP, DW, DH, Ms[k]);
      for (int y = 0; y < DH; ++y)
        for (int x = 0; x < DP; ++x) {
          const int want = x >= DW ? 0xA5 : (k == 0 ? src[0] : 0);
          if (dst[y * DP + x] != want) {
            fprintf(stderr, "warp %d at (%d, %d): %d\n", k, x, y, dst[y * DP + x]);
            ++fails;
            y = DH;
            break;
          }
        }
    }
  }
  /* frame1 200 x 160 against frame0 260 x 190 and the other way round, pitched crops of one
   * noise field 14 px and 9 px apart */
  {
    enum { BW = 300, BH = 220 };
    uint8_t *base = malloc(BW * BH);
    noise(BW, BH, BW, 21u, base);
    float aff[6];
    int ng = -1, oc = -1;
    const int rc = orc_find_alignment(base + 9 * BW + 14, BW, 200, 160, base, BW, 260, 190, &kOrb, aff, &ng, &oc);
    const int rs = orc_find_alignment(base, BW, 260, 190, base + 9 * BW + 14, BW, 200, 160, &kOrb, aff, &ng, &oc);
    if (rc != 0 || rs != 0 || oc != 0 || ng <= 10) {
      fprintf(stderr, "find_alignment: status %d / %d, %d good, outcome %d\n", rc, rs, ng, oc);
      ++fails;
    }
    free(base);
  }
  return fails;
}

/* profile 1: the exact-2x pyramid on odd levels, with and without gamma and the median, u8
 * and f32 frames; tiny frames under every median size */
static int dualtvl1_edges(void) {
  static const int odd[][2] = {{35, 36}, {36, 35}, {35, 35}, {39, 67}, {70, 70}, {33, 37}};
  static const int tiny[][2] = {{1, 1}, {1, 2}, {2, 1}, {2, 2}, {3, 3}, {1, 3}, {3, 1},
                                {4, 5}, {5, 4}, {1, 64}, {64, 1}, {2, 65}};
  static const int medians[] = {1, 3, 5};
  int fails = 0;
  /* 19 x 67 -> 10 x 34 (too small for a pyramid level): the 2x path alone, into exact buffers */
  {
    enum { SW = 19, SH = 67, DW = 10, DH = 34 };
    float *src = malloc(sizeof(float) * SW * SH), *dst = malloc(sizeof(float) * DW * DH);
    for (int i = 0; i < SW * SH; ++i) src[i] = 1.0f;
    orc_resize_hp(src, SW, SH, dst, DW, DH, 2.0, 2.0, 1);
    for (int i = 0; i < DW * DH; ++i)
      if (dst[i] != 1.0f) {
        fprintf(stderr, "2x resize of a constant 19x67: %g at %d\n", dst[i], i);
        ++fails;
        break;
      }
    free(src);
    free(dst);
  }
  for (size_t si = 0; si < sizeof odd / sizeof odd[0] + sizeof tiny / sizeof tiny[0]; ++si) {
    const int is_odd = si < sizeof odd / sizeof odd[0];
    const int *sz = is_odd ? odd[si] : tiny[si - sizeof odd / sizeof odd[0]];
    const int w = sz[0], h = sz[1];
    uint8_t *a = malloc((size_t)w * h), *b = malloc((size_t)w * h);
    float *fa = malloc(sizeof(float) * w * h), *fb = malloc(sizeof(float) * w * h);
    float *u = malloc(sizeof(float) * w * h), *v = malloc(sizeof(float) * w * h);
    pair(w, h, 101u + (unsigned)si, a, b);
    for (int i = 0; i < w * h; ++i) fa[i] = (float)a[i] / 255.0f, fb[i] = (float)b[i] / 255.0f;
    for (int variant = 0; variant < 4; ++variant) {
      tvl1_params p = {0.25, 0.15, 0.3, 3, 2, 0.01, 300, 0.5, 0.0, 0, 1, 0, 1, 3, 2};
      if (is_odd) {
        if (variant == 1) p.gamma = 0.2;
        if (variant == 2) p.median_filtering = 5, p.nscales = 4;
      } else {
        if (variant == 3) continue;
        p.median_filtering = medians[variant], p.nscales = 1, p.scale_step = 0.8, p.warps = 3;
      }
      int32_t wi[32 * 3];
      tvl1_stats st;
      memset(&st, 0, sizeof st);
      st.warp_iterations = wi;
      st.warp_iterations_capacity = 32 * 3;
      const int rc = variant == 3 ? orc_tvl1_calc_f32(&p, fa, sizeof(float) * (size_t)w, fb,
                                                      sizeof(float) * (size_t)w, w, h, u, v,
                                                      sizeof(float) * (size_t)w, &st)
                                  : orc_tvl1_calc(&p, a, (size_t)w, b, (size_t)w, w, h, u, v,
                                                  sizeof(float) * (size_t)w, &st);
      if (rc != 0 || (is_odd && st.levels < 2) || st.checks_total != st.iterations_total) {
        fprintf(stderr, "profile 1 %dx%d variant %d: status %d, %d levels\n", w, h, variant, rc, st.levels);
        ++fails;
      }
    }
    free(a);
    free(b);
    free(fa);
    free(fb);
    free(u);
    free(v);
  }
  return fails;
}

int main(void) {
  static const int sizes[][2] = {{1, 1}, {16, 16}, {17, 16}, {33, 19}, {61, 47}, {97, 40}};
  int fails = 0;
  for (size_t si = 0; si < sizeof sizes / sizeof sizes[0]; ++si) {
    const int w = sizes[si][0], h = sizes[si][1];
    uint8_t *a = malloc((size_t)w * h), *b = malloc((size_t)w * h);
    float *u = malloc(sizeof(float) * w * h), *v = malloc(sizeof(float) * w * h);
    pair(w, h, 7u + (unsigned)si, a, b);
    for (int variant = 0; variant < 6; ++variant) {
      tvl1_params p = {0.25, 0.05, 0.3, 10, 3, 0.01, 300, 0.8, 0.0, 0, 1, 0, 0, 30, 10};
      if (variant == 1) p.gamma = 0.2;
      if (variant == 2) p.median_filtering = 5;
      if (variant == 3) p.epsilon = 0.0, p.iterations = 7;
      if (variant == 4) p.profile = 1, p.lambda = 0.15, p.nscales = 3, p.inner_iterations = 5,
                        p.outer_iterations = 2, p.median_filtering = 5;
      if (variant == 5) p.scale_step = 0.5;
      int32_t wi[32 * 3];
      tvl1_stats st;
      memset(&st, 0, sizeof st);
      st.warp_iterations = wi;
      st.warp_iterations_capacity = 32 * 3;
      const int rc = orc_tvl1_calc(&p, a, (size_t)w, b, (size_t)w, w, h, u, v,
                                   sizeof(float) * (size_t)w, &st);
      if (rc != 0) {
        fprintf(stderr, "%dx%d variant %d: status %d\n", w, h, variant, rc);
        ++fails;
      }
      orc_postprocess(u, v, sizeof(float) * (size_t)w, b, (size_t)w, w, h, 1);
    }
    /* orc_tvl1_calc_init: IEEE and fma, seed rows padded by 3 floats, flows past every edge */
    const size_t sp = (size_t)w + 3;
    float *u0 = malloc(sizeof(float) * sp * h), *v0 = malloc(sizeof(float) * sp * h);
    for (int y = 0; y < h; ++y)
      for (size_t x = 0; x < sp; ++x) {
        u0[y * sp + x] = (float)((int)((x * 7 + (size_t)y * 3) % 23) - 11) * 0.75f;
        v0[y * sp + x] = (float)((int)((x * 5 + (size_t)y * 11) % 19) - 9) * 1.25f;
      }
    for (int fm = 0; fm <= 2; fm += 2) {
      tvl1_params p = {0.25, 0.05, 0.3, 10, 3, 0.01, 300, 0.8, 0.0, 0, 1, 0, 0, 30, 10};
      p.fast_math = fm;
      tvl1_stats st;
      memset(&st, 0, sizeof st);
      const int rc = orc_tvl1_calc_init(&p, a, (size_t)w, b, (size_t)w, w, h, u0, v0,
                                        sizeof(float) * sp, u, v, sizeof(float) * (size_t)w, &st);
      p.profile = 1;
      const int rc1 = orc_tvl1_calc_init(&p, a, (size_t)w, b, (size_t)w, w, h, u0, v0,
                                         sizeof(float) * sp, u, v, sizeof(float) * (size_t)w, &st);
      if (rc != 0 || rc1 != TVL1_EINVAL) {
        fprintf(stderr, "%dx%d seeded fast_math %d: status %d, profile 1: %d\n", w, h, fm, rc, rc1);
        ++fails;
      }
    }
    /* the fast branch: unseeded (stopping rule, median, fixed work), seeded, f32 frames; a
     * primitive that fails on its 1st .. 4th call; then uninstalled (IEEE, no call) */
    {
      float *fa = malloc(sizeof(float) * w * h), *fb = malloc(sizeof(float) * w * h);
      for (int i = 0; i < w * h; ++i) fa[i] = (float)a[i] / 255.0f, fb[i] = (float)b[i] / 255.0f;
      orc_set_approx_prims(rcp_c, sqrt_c);
      for (int variant = 0; variant < 9; ++variant) {
        tvl1_params p = {0.25, 0.05, 0.3, 10, 3, 0.01, 300, 0.8, 0.0, 0, 1, 1, 0, 30, 10};
        if (variant == 1) p.median_filtering = 3;
        if (variant == 2) p.epsilon = 0.0, p.iterations = 3;
        g_prim_calls = 0;
        g_prim_fail = variant >= 5 ? variant - 5 : -1;
        tvl1_stats st;
        memset(&st, 0, sizeof st);
        int rc;
        if (variant == 3)
          rc = orc_tvl1_calc_init(&p, a, (size_t)w, b, (size_t)w, w, h, u0, v0, sizeof(float) * sp,
                                  u, v, sizeof(float) * (size_t)w, &st);
        else if (variant == 4)
          rc = orc_tvl1_calc_f32(&p, fa, sizeof(float) * (size_t)w, fb, sizeof(float) * (size_t)w,
                                 w, h, u, v, sizeof(float) * (size_t)w, &st);
        else
          rc = orc_tvl1_calc(&p, a, (size_t)w, b, (size_t)w, w, h, u, v,
                             sizeof(float) * (size_t)w, &st);
        const int want = variant >= 5 ? TVL1_EHIP : TVL1_OK;
        if (rc != want || g_prim_calls == 0 ||
            (rc == TVL1_OK && g_prim_calls != 2 * (int)st.iterations_total + 2 * p.warps * st.levels)) {
          fprintf(stderr, "%dx%d fast variant %d: status %d, %d primitive calls\n", w, h, variant,
                  rc, g_prim_calls);
          ++fails;
        }
      }
      orc_set_approx_prims(NULL, NULL);
      g_prim_calls = 0, g_prim_fail = -1;
      tvl1_params p = {0.25, 0.05, 0.3, 10, 3, 0.01, 300, 0.8, 0.0, 0, 1, 1, 0, 30, 10};
      const int rc = orc_tvl1_calc(&p, a, (size_t)w, b, (size_t)w, w, h, u, v,
                                   sizeof(float) * (size_t)w, NULL);
      if (rc != 0 || g_prim_calls != 0) {
        fprintf(stderr, "%dx%d fast uninstalled: status %d, %d primitive calls\n", w, h, rc, g_prim_calls);
        ++fails;
      }
      free(fa);
      free(fb);
    }
    free(u0);
    free(v0);
    free(a);
    free(b);
    free(u);
    free(v);
  }
  fails += align_paths();
  fails += dualtvl1_edges();
  printf("oracle asan driver: %d failures\n", fails);
  return fails != 0;
}
