// Per-sample gradients -> per-ray gradients (fenerf_ray_grads / fenerf_render_backward_rays, include/fenerf.h): the backward of
//     points = origins + dirs * z,  per-sample view direction = dirs                    (generators.py:468-476, :504)
// for depths z that are constants of the graph (generators.py:465, :483-503 run under torch.no_grad()):
//     d_origins[ray] = sum_pass sum_n d_points[pass][ray][n]
//     d_dirs[ray]    = sum_pass sum_n z[pass][ray][n] * d_points[pass][ray][n]  +  sum_pass sum_n d_viewdirs[pass][ray][n]
// What torch autograd's broadcast sums leave in origins.grad / dirs.grad -- as one launch after fenerf_siren_input_grads has filled the
// per-sample buffers.
#include <hip/hip_runtime.h>

#include "fenerf_internal.h"

namespace fenerf {

// One lane owns one ray and walks its samples in order: coarse n ascending, then fine n ascending, one fp32 add (origins, view
// directions) or one fp32 FMA (z * d_points) per sample and component.  The order of a ray's additions is therefore the same for every
// grid size, and there is no cross-lane step and no atomic.  HBM-bound and small (passes * N * 28 bytes per ray): a lane reads its ray's
// samples as one contiguous run of 12 N bytes per buffer, so every line a wave fetches is consumed by that wave within the next
// iterations; the loop is unrolled four deep to keep that many samples' loads in flight per lane.  Rows P .. Pp - 1 of an image (the
// pad of the 32-point tiles) are never addressed: the last ray ends at row R N - 1.
__global__ __launch_bounds__(64) void ray_grad_reduce_kernel(const float* __restrict__ d_pts2, const float* __restrict__ d_rd2,
                                                              const float* __restrict__ z_coarse, const float* __restrict__ z_fine,
                                                              float* __restrict__ d_origins, float* __restrict__ d_dirs, int B, int R, int N,
                                                              long long Pp, int passes) {
  const long long rays = (long long)B * R;
  for (long long ray = (long long)blockIdx.x * blockDim.x + threadIdx.x; ray < rays; ray += (long long)gridDim.x * blockDim.x) {
    const long long b = ray / R, r = ray % R;
    float ox = 0.f, oy = 0.f, oz = 0.f;       // sum d_points
    float zx = 0.f, zy = 0.f, zz = 0.f;       // sum z * d_points
    float vx = 0.f, vy = 0.f, vz = 0.f;       // sum d_viewdirs
    for (int pass = 0; pass < passes; ++pass) {
      const long long row0 = ((long long)pass * B + b) * Pp + r * N;
      const float* dp = d_pts2 + row0 * 3;
      const float* dv = d_rd2 ? d_rd2 + row0 * 3 : nullptr;
      const float* z = (pass == 0 ? z_coarse : z_fine) + ray * N;
#pragma unroll 4
      for (int n = 0; n < N; ++n) {
        const float gx = dp[3 * n + 0], gy = dp[3 * n + 1], gz = dp[3 * n + 2];
        ox += gx; oy += gy; oz += gz;
        if (d_dirs) {
          const float t = z[n];
          zx = fmaf(t, gx, zx); zy = fmaf(t, gy, zy); zz = fmaf(t, gz, zz);
          if (dv) { vx += dv[3 * n + 0]; vy += dv[3 * n + 1]; vz += dv[3 * n + 2]; }
        }
      }
    }
    if (d_origins) { d_origins[ray * 3 + 0] = ox; d_origins[ray * 3 + 1] = oy; d_origins[ray * 3 + 2] = oz; }
    if (d_dirs) { d_dirs[ray * 3 + 0] = zx + vx; d_dirs[ray * 3 + 1] = zy + vy; d_dirs[ray * 3 + 2] = zz + vz; }
  }
}

int launch_ray_grads(int B, int R, int N, long long Pp, int passes, const float* d_pts2, const float* d_rd2, const float* z_coarse,
                     const float* z_fine, float* d_origins, float* d_dirs, void* stream) {
  const long long rays = (long long)B * R;
  // one wave per workgroup: a 128 x 128 image is 256 waves, one per compute unit instead of four on every fourth
  long long bx = (rays + 63) / 64;
  if (bx > 8192) bx = 8192;
  hipLaunchKernelGGL(ray_grad_reduce_kernel, dim3((unsigned)bx), dim3(64), 0, (hipStream_t)stream, d_pts2, d_rd2, z_coarse, z_fine, d_origins, d_dirs,
                     B, R, N, Pp, passes);
  return check_launch("ray gradient launch");
}

}  // namespace fenerf
