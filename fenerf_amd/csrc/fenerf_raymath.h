// Pixel-grid and depth arithmetic shared by the kernels that make rays: ray_setup_kernel (fenerf_composite.hip) and camera_rays_kernel
// (fenerf_camera.hip).  Every operation is rounded on its own unless stated: the two kernels give the same bits for the same camera.
#pragma once
#include <hip/hip_runtime.h>

namespace fenerf {

// torch.linspace kernel: step = (end-start)/(steps-1); i < steps/2 ? start + step*i : end - step*(steps-1-i).
// FUSED: each of the two as ONE fused multiply-add, a single rounding -- what torch's builds contract them into (x86 with AVX2 / AVX-512).
// The sample depths are FUSED: the depths the reference recorded (tests/golden, 24 samples) are those bits, and a separately rounded product
// is one ulp off at sample 9 of every ray (at sample 5 of 12 in (0.1, 5)).
// The pixel grid is NOT fused and so DIFFERS FROM TORCH, by one ulp at about half of its values (124 of linspace(-1, 1, 256)): torch fuses
// it like the depths.  Known and left for a change of its own: the rays of the 128 x 128, 24 + 24 image move with it, and the flip
// statistics that tests/test_gpu_parity.py pins on that image (test_resampling_flips_against_an_fp64_arbiter) have to be measured again.
template <bool FUSED>
__device__ __forceinline__ float torch_linspace(float start, float end, int steps, int i) {
  if (steps == 1) return start;
  const float step = __fdiv_rn(__fsub_rn(end, start), (float)(steps - 1));
  if (FUSED) return i < steps / 2 ? __fmaf_rn(step, (float)i, start) : __fmaf_rn(-step, (float)(steps - 1 - i), end);
  return i < steps / 2 ? __fadd_rn(start, __fmul_rn(step, (float)i)) : __fsub_rn(end, __fmul_rn(step, (float)(steps - 1 - i)));
}
__device__ __forceinline__ void normalize3(float& x, float& y, float& z) {
  const float n = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z)));
  x = __fdiv_rn(x, n); y = __fdiv_rn(y, n); z = __fdiv_rn(z, n);
}

// stratified jitter (volumetric_rendering.py:133-139): z_k = linspace(start,end,N)[k] + (u - 0.5) * (z_1 - z_0), for one ray's N samples
__device__ __forceinline__ void jittered_depths(float ray_start, float ray_end, int N, const float* __restrict__ u, float* __restrict__ z) {
  const float step = N > 1 ? __fsub_rn(torch_linspace<true>(ray_start, ray_end, N, 1), torch_linspace<true>(ray_start, ray_end, N, 0)) : 0.f;
  for (int k = 0; k < N; ++k)
    z[k] = __fadd_rn(torch_linspace<true>(ray_start, ray_end, N, k), __fmul_rn(__fsub_rn(u[k], 0.5f), step));
}

}  // namespace fenerf
