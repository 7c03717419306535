// TEST INFRASTRUCTURE ONLY: the two approximate instructions of the engine's fast mode
// (v_rcp_f32, v_sqrt_f32; csrc/tvl1_kernels.hpp's approx(FM) sites) as element-wise kernels
// behind host functions of tvl1_oracle.h's orc_vec_fn shape, so the oracle's fast branch
// can ask the hardware for them (orc_set_approx_prims).  Built with the engine's flags
// (oracle/Makefile), so the kernels' float mode is the engine's.  liboracle_tvl1.so does not
// link this library: oracle/checker.py hands the two function addresses from one to the other.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>

namespace {

__global__ __launch_bounds__(256) void k_rcp(const float *__restrict__ in, float *__restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = __builtin_amdgcn_rcpf(in[i]);
}

__global__ __launch_bounds__(256) void k_sqrt(const float *__restrict__ in, float *__restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = __builtin_amdgcn_sqrtf(in[i]);
}

// device scratch for one input and one output plane; only ever grown
float *g_in = nullptr, *g_out = nullptr;
size_t g_cap = 0;

bool failed(hipError_t e, const char *what) {
  if (e == hipSuccess) return false;
  std::fprintf(stderr, "fast_prims: %s: %s\n", what, hipGetErrorString(e));
  return true;
}

bool reserve(size_t n) {
  if (n <= g_cap) return true;
  if (g_in && failed(hipFree(g_in), "hipFree")) return false;
  if (g_out && failed(hipFree(g_out), "hipFree")) return false;
  g_in = g_out = nullptr;
  g_cap = 0;
  if (failed(hipMalloc(&g_in, n * sizeof(float)), "hipMalloc")) return false;
  if (failed(hipMalloc(&g_out, n * sizeof(float)), "hipMalloc")) {
    (void)hipFree(g_in);
    g_in = nullptr;
    return false;
  }
  g_cap = n;
  return true;
}

// host array in, one launch, host array out, on device 0, synchronously
template <typename K>
int run(K kernel, const float *in, float *out, size_t n) {
  if (n == 0) return 0;
  if (!in || !out || n > ((size_t)1 << 31)) return 1;
  if (failed(hipSetDevice(0), "hipSetDevice")) return 1;
  if (!reserve(n)) return 1;
  if (failed(hipMemcpy(g_in, in, n * sizeof(float), hipMemcpyHostToDevice), "copy in")) return 1;
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, 0, g_in, g_out, n);
  if (failed(hipGetLastError(), "launch")) return 1;
  if (failed(hipDeviceSynchronize(), "synchronize")) return 1;
  if (failed(hipMemcpy(out, g_out, n * sizeof(float), hipMemcpyDeviceToHost), "copy out")) return 1;
  return 0;
}

}  // namespace

extern "C" {
int fastprims_rcp(const float *in, float *out, size_t n) { return run(k_rcp, in, out, n); }
int fastprims_sqrt(const float *in, float *out, size_t n) { return run(k_sqrt, in, out, n); }
}
