// stages_plan_dump: the k_iterate_stages planner (csrc/tvl1_plan.hpp) for
// tests/test_stages_plan_cpu.py.  Plain C++17, no HIP.  One output line per input line
//   W H K slots roll_seg p_zero
// -> bands seg_rows waves out_w halo hbm_bytes partials_capacity nseg {ys ye r0 steps} x nseg
#include <cstdio>

#include "tvl1_plan.hpp"

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  int W, H, K, slots, roll_seg, pz;
  while (fscanf(f, "%d %d %d %d %d %d", &W, &H, &K, &slots, &roll_seg, &pz) == 6) {
    const tvl1k::StreamPlan p = tvl1k::plan_stages(W, H, K, slots, roll_seg);
    const double hbm = tvl1k::stages_hbm(p, H, K, (double)W * H, tvl1k::pass_planes(false, pz != 0));
    const int nseg = (H + p.seg_rows - 1) / p.seg_rows;
    printf("%d %d %d %d %d %.0f %d %d", p.bands, p.seg_rows, p.waves, tvl1k::stages_out_w(K),
           tvl1k::roll_halo_of(K, 2), hbm, tvl1k::partials_capacity(W, H), nseg);
    for (int s = 0; s < nseg; ++s) {
      const int ys = s * p.seg_rows, ye = ys + p.seg_rows < H ? ys + p.seg_rows : H;
      printf(" %d %d %d %d", ys, ye, tvl1k::stages_r0(ys, K), tvl1k::stages_steps(ys, ye, K));
    }
    printf("\n");
  }
  fclose(f);
  return 0;
}
