// Free camera (fenerf_camera_rays / fenerf_camera_grads, include/fenerf.h): the rays of a window of a W x H pixel grid from a
// camera-to-world matrix and five intrinsics per image, and the reduction of per-ray gradients to the gradients of those 17 numbers.
//
//   pixel (col, row):  X = linspace(-1, 1, W)[col],  Y = linspace(1, -1, H)[row]          (the grid of ray_setup_kernel, fenerf_raymath.h)
//   v = (kx (X - cx), ky (Y - cy), zc),  c = v / |v|,  dirs = M[:, :3] c,  origins = M[:, 3]
//
// The reference has one camera (volumetric_rendering.py:109-168, :220-248: on the unit sphere, looking at the origin, square image);
// it is intrinsics = (1, 1, 0, 0, -1 / tan(fov / 2)) with the look-at matrix, and ray_setup_kernel's bits.
#include <hip/hip_runtime.h>

#include "fenerf_internal.h"
#include "fenerf_lane.h"
#include "fenerf_raymath.h"

namespace fenerf {

struct CameraGrid { int B, W, H, x0, y0, w, h; };

// the full-grid pixel of ray r of a window, and its grid coordinates
__device__ __forceinline__ void window_pixel(const CameraGrid& g, int r, float& X, float& Y) {
  const int col = g.x0 + r % g.w, row = g.y0 + r / g.w;
  X = torch_linspace<false>(-1.f, 1.f, g.W, col);
  Y = torch_linspace<false>(1.f, -1.f, g.H, row);
}

// One thread per ray, as ray_setup_kernel; the 17 camera numbers of an image are wave-uniform loads from L2.
__global__ __launch_bounds__(256) void camera_rays_kernel(CameraGrid g, int N, const float* __restrict__ cam2world,
                                                          const float* __restrict__ intrinsics, float ray_start, float ray_end,
                                                          const float* __restrict__ u_jitter, float* __restrict__ origins,
                                                          float* __restrict__ dirs, float* __restrict__ z_out) {
  const long long R = (long long)g.w * g.h;
  const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (idx >= (long long)g.B * R) return;
  const int b = (int)(idx / R);
  const int r = (int)(idx % R);
  const float* M = cam2world + (long long)b * 12;
  const float* K = intrinsics + (long long)b * 5;
  float X, Y;
  window_pixel(g, r, X, Y);
  float cx = __fmul_rn(K[0], __fsub_rn(X, K[2])), cy = __fmul_rn(K[1], __fsub_rn(Y, K[3])), cz = K[4];
  normalize3(cx, cy, cz);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    dirs[idx * 3 + i] = __fadd_rn(__fadd_rn(__fmul_rn(M[4 * i + 0], cx), __fmul_rn(M[4 * i + 1], cy)), __fmul_rn(M[4 * i + 2], cz));
    origins[idx * 3 + i] = M[4 * i + 3];
  }
  jittered_depths(ray_start, ray_end, N, u_jitter + idx * N, z_out + idx * N);
}

int launch_camera_rays(int B, int W, int H, int x0, int y0, int w, int h, int N, const float* cam2world, const float* intrinsics,
                       float ray_start, float ray_end, const float* u_jitter, float* origins, float* dirs, float* z, void* stream) {
  const long long total = (long long)B * w * h;
  if (total <= 0) return FENERF_OK;
  const CameraGrid g{B, W, H, x0, y0, w, h};
  hipLaunchKernelGGL(camera_rays_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, N, cam2world,
                     intrinsics, ray_start, ray_end, u_jitter, origins, dirs, z);
  return check_launch("camera_rays launch");
}

// ------------------------------------------------------------------------------------------------
// backward: 17 sums over the R rays of each image, in a fixed order and without atomics
// ------------------------------------------------------------------------------------------------
// Stage 1, grid (G, B), 256 lanes: workgroup g owns rays [256 k g, 256 k (g + 1)) of its image; lane t adds the terms of rays
// 256 k g + 256 j + t, j = 0 .. k - 1 (k additions, coalesced reads), wave_sum adds the 64 lanes (6), lane 0 of each of the four waves
// leaves its sum in LDS and 17 lanes add those in wave order (3) -> partial[b][g][17].
// Stage 2, grid (17, B), one wave: lane l adds partial[b][g][o] for g = l, l + 64, ... in index order (ceil(G / 64) additions), then
// wave_sum (6).
// G = min(256, ceil(R / 1024)) and k = ceil(R / (256 G)): four rays per lane until 256 workgroups per image are reached (R = 2^18), more
// rays per lane after that.  The number of additions one term passes through is therefore at most
//     L(R) = k + 6 + 3 + ceil(G / 64) + 6                (camera_grads_chain_length: at most 20 for R <= 1024, 35 at R = 2^20)
// which stays within 64 up to R = 45 * 2^16 (k = 45) and grows as R / 2^16 beyond.
constexpr int CG_LANES = 256, CG_WAVES = CG_LANES / 64, CG_TERMS = 17, CG_MAX_GROUPS = 256, CG_RAYS_PER_LANE = 4;

int camera_grads_groups(long long R) {
  const long long per = (long long)CG_LANES * CG_RAYS_PER_LANE;
  const long long G = (R + per - 1) / per;
  return (int)(G < 1 ? 1 : G > CG_MAX_GROUPS ? CG_MAX_GROUPS : G);
}
static int camera_grads_rays_per_lane(long long R) {
  const long long per = (long long)CG_LANES * camera_grads_groups(R);
  return (int)((R + per - 1) / per);
}
int camera_grads_chain_length(long long R) {
  return camera_grads_rays_per_lane(R) + 6 + (CG_WAVES - 1) + (camera_grads_groups(R) + 63) / 64 + 6;
}

__global__ __launch_bounds__(CG_LANES) void camera_grads_partial_kernel(CameraGrid g, int k, const float* __restrict__ cam2world,
                                                                        const float* __restrict__ intrinsics,
                                                                        const float* __restrict__ d_origins,
                                                                        const float* __restrict__ d_dirs, float* __restrict__ partial) {
  __shared__ float s_sum[CG_WAVES][CG_TERMS];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long R = (long long)g.w * g.h;
  const float* M = cam2world + (long long)b * 12;
  const float* K = intrinsics + (long long)b * 5;
  const float kx = K[0], ky = K[1], ccx = K[2], ccy = K[3], zc = K[4];
  float acc[CG_TERMS];
#pragma unroll
  for (int o = 0; o < CG_TERMS; ++o) acc[o] = 0.f;
  const long long first = (long long)blockIdx.x * CG_LANES * k + tid;
  for (int j = 0; j < k; ++j) {
    const long long r = first + (long long)j * CG_LANES;
    if (r >= R) break;
    const long long ray = (long long)b * R + r;
    if (d_origins) {
#pragma unroll
      for (int i = 0; i < 3; ++i) acc[4 * i + 3] += d_origins[ray * 3 + i];
    }
    if (d_dirs) {
      float X, Y;
      window_pixel(g, (int)r, X, Y);
      const float xs = X - ccx, ys = Y - ccy;
      const float vx = kx * xs, vy = ky * ys, vz = zc;
      const float sx = vx * vx, sy = vy * vy, sz = vz * vz, n2 = sx + sy + sz;
      const float n = sqrtf(n2);
      const float c[3] = {vx / n, vy / n, vz / n};
      const float dd[3] = {d_dirs[ray * 3 + 0], d_dirs[ray * 3 + 1], d_dirs[ray * 3 + 2]};
      float gc[3];   // M[:, :3]^T d_dirs: the gradient wrt c
#pragma unroll
      for (int jc = 0; jc < 3; ++jc) gc[jc] = M[jc] * dd[0] + M[4 + jc] * dd[1] + M[8 + jc] * dd[2];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int jc = 0; jc < 3; ++jc) acc[4 * i + jc] += dd[i] * c[jc];
      // gv = (g - c (c . g)) / n, the gradient wrt v, as (g |v|^2 - v (v . g)) / n^3 with |v|^2 - v_i^2 written as the other two squares:
      // near the image centre c is almost (0, 0, -1) and g.z - c.z (c . g) would be the small difference of two values of g's size
      const float inv_n3 = 1.f / (n2 * n);
      const float gvx = (gc[0] * (sy + sz) - vx * (vy * gc[1] + vz * gc[2])) * inv_n3;
      const float gvy = (gc[1] * (sx + sz) - vy * (vx * gc[0] + vz * gc[2])) * inv_n3;
      const float gvz = (gc[2] * (sx + sy) - vz * (vx * gc[0] + vy * gc[1])) * inv_n3;
      acc[12] += gvx * xs;        // d kx
      acc[13] += gvy * ys;        // d ky
      acc[14] += -(gvx * kx);     // d cx
      acc[15] += -(gvy * ky);     // d cy
      acc[16] += gvz;             // d zc
    }
  }
#pragma unroll
  for (int o = 0; o < CG_TERMS; ++o) {
    const float s = wave_sum(acc[o]);
    if (lane == 0) s_sum[wv][o] = s;
  }
  __syncthreads();
  if (tid < CG_TERMS) {
    float s = s_sum[0][tid];
#pragma unroll
    for (int q = 1; q < CG_WAVES; ++q) s += s_sum[q][tid];
    partial[((long long)b * gridDim.x + blockIdx.x) * CG_TERMS + tid] = s;
  }
}

__global__ __launch_bounds__(64) void camera_grads_final_kernel(int G, const float* __restrict__ partial, float* __restrict__ d_cam2world,
                                                                float* __restrict__ d_intrinsics) {
  const int o = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const float* p = partial + (long long)b * G * CG_TERMS + o;
  float s = 0.f;
  for (int gi = lane; gi < G; gi += 64) s += p[(long long)gi * CG_TERMS];
  s = wave_sum(s);
  if (lane == 0) {
    if (o < 12) d_cam2world[(long long)b * 12 + o] = s;
    else d_intrinsics[(long long)b * 5 + (o - 12)] = s;
  }
}

int launch_camera_grads(int B, int W, int H, int x0, int y0, int w, int h, const float* cam2world, const float* intrinsics,
                        const float* d_origins, const float* d_dirs, float* d_cam2world, float* d_intrinsics, float* partial, void* stream) {
  const long long R = (long long)w * h;
  const int G = camera_grads_groups(R), k = camera_grads_rays_per_lane(R);
  const CameraGrid g{B, W, H, x0, y0, w, h};
  hipLaunchKernelGGL(camera_grads_partial_kernel, dim3((unsigned)G, (unsigned)B), dim3(CG_LANES), 0, (hipStream_t)stream, g, k, cam2world,
                     intrinsics, d_origins, d_dirs, partial);
  int rc = check_launch("camera_grads partial launch");
  if (rc) return rc;
  hipLaunchKernelGGL(camera_grads_final_kernel, dim3(CG_TERMS, (unsigned)B), dim3(64), 0, (hipStream_t)stream, G, partial, d_cam2world,
                     d_intrinsics);
  return check_launch("camera_grads final launch");
}

}  // namespace fenerf
