// Geometry views (include/fenerf.h "geometry views"): the surface point of a ray, the density gradient of a baked lattice, and normals with
// Lambert shading.  fenerf_amd/geometry_emulation.py restates the arithmetic in numpy; tests compare bit for bit.
// Three stand-alone kernels, one thread per output row, 256 threads (four wave64) per workgroup:
//   surface_points      lane = (image, padded row): z = depth or depth / alpha, p = origin + dir * z; rows R .. Pp - 1 of an image repeat
//                       the point of its ray R - 1, so the result feeds the differentiable SIREN calls (whole 32-point tiles) as it is;
//   volume_sample_grad  lane = point: the sampler's cell and fractions, then per axis the trilinear value of ONE channel one cell ahead
//                       and one cell behind with the point's own fractions (2 x 8 dword loads, 2 x 7 lerps), their difference over two
//                       spacings.  Only interior cells are differenced, so every address lies inside the lattice by construction;
//   shade_normals       lane = ray: n = -g / |g|, optionally into camera space, Lambert + ambient, alpha-blended onto the background.
// Every fp32 operation is rounded on its own (the _rn intrinsics, and -ffp-contract=off).  Addresses come from integer indices alone.
// No atomics, no LDS, no workgroup waits for another: the same bytes on every run.  The C-ABI entries are at the end of this file.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "fenerf_internal.h"

namespace fenerf {

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ float lerp_rn(float a, float b, float f) {
  return __fadd_rn(__fmul_rn(a, __fsub_rn(1.f, f)), __fmul_rn(b, f));
}

struct SurfaceParams {
  int B, R;
  long long Pp;            // rows per image of `points`: R rounded up to a multiple of 32
  const float* origins;    // [B*R][3]
  const float* dirs;       // [B*R][3]
  const float* depth;      // [B*R]
  const float* alpha;      // [B*R] or nullptr
  float alpha_min;
  float* points;           // [B][Pp][3]
};

__global__ void __launch_bounds__(kThreads) surface_points_kernel(const SurfaceParams p) {
  const long long row = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (row >= (long long)p.B * p.Pp) return;
  const long long b = row / p.Pp, r = row - b * p.Pp;
  const long long ray = b * p.R + (r < p.R ? r : p.R - 1);
  float z = p.depth[ray];
  if (p.alpha) {
    const float a = p.alpha[ray];
    if (a >= p.alpha_min) z = __fdiv_rn(z, a);          // ordered: false for NaN
  }
  for (int k = 0; k < 3; ++k) p.points[row * 3 + k] = __fadd_rn(p.origins[ray * 3 + k], __fmul_rn(p.dirs[ray * 3 + k], z));
}

struct VolumeGradParams {
  const float* vol;        // [n0][n1][n2][ld]
  int n0, n1, n2, ld, channel;
  float origin[3], spacing[3];
  long long P;
  const float* points;     // [P][3]
  float* grads;            // [P][3]
};

// the sampler's step-4 value of one channel at cell (i0, i1, i2) with fractions f: corner d0 d1 d2 at base + d0 s0 + d1 s1 + d2 s2
__device__ __forceinline__ float cell_value(const float* base, long long s0, long long s1, long long s2, float f0, float f1, float f2) {
  const float c00 = lerp_rn(base[0], base[s2], f2), c01 = lerp_rn(base[s1], base[s1 + s2], f2);                           // axis 2
  const float c10 = lerp_rn(base[s0], base[s0 + s2], f2), c11 = lerp_rn(base[s0 + s1], base[s0 + s1 + s2], f2);
  const float c0 = lerp_rn(c00, c01, f1), c1 = lerp_rn(c10, c11, f1);                                                     // axis 1
  return lerp_rn(c0, c1, f0);                                                                                             // axis 0
}

__global__ void __launch_bounds__(kThreads) volume_sample_grad_kernel(const VolumeGradParams p) {
  const long long s = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (s >= p.P) return;
  const int n[3] = {p.n0, p.n1, p.n2};
  int i[3] = {0, 0, 0};
  float f[3] = {0.f, 0.f, 0.f};
  bool interior = true;
  for (int k = 0; k < 3; ++k) {
    const float t = __fdiv_rn(__fsub_rn(p.points[s * 3 + k], p.origin[k]), p.spacing[k]);
    const bool inside = t >= 0.f && t <= (float)(n[k] - 1);          // ordered: false for NaN
    if (inside) {
      i[k] = min((int)floorf(t), n[k] - 2);
      f[k] = __fsub_rn(t, (float)i[k]);
    }
    interior = interior && inside && i[k] >= 1 && i[k] <= n[k] - 3;
  }
  float g[3] = {0.f, 0.f, 0.f};
  if (interior) {
    const long long stride[3] = {(long long)p.n1 * p.n2 * p.ld, (long long)p.n2 * p.ld, (long long)p.ld};       // in floats
    const float* base = p.vol + ((long long)i[0] * p.n1 + i[1]) * p.n2 * p.ld + (long long)i[2] * p.ld + p.channel;
    for (int k = 0; k < 3; ++k) {
      const float ahead = cell_value(base + stride[k], stride[0], stride[1], stride[2], f[0], f[1], f[2]);
      const float behind = cell_value(base - stride[k], stride[0], stride[1], stride[2], f[0], f[1], f[2]);
      g[k] = __fdiv_rn(__fsub_rn(ahead, behind), __fadd_rn(p.spacing[k], p.spacing[k]));
    }
  }
  for (int k = 0; k < 3; ++k) p.grads[s * 3 + k] = g[k];
}

struct ShadeParams {
  int B, R;
  long long rows_per_image;
  const float* grads;      // [B][rows_per_image][3]
  const float* alpha;      // [B*R] or nullptr
  const float* cam2world;  // [B][3][3] row-major or nullptr
  float light[3];
  float ambient, background, alpha_min;
  float* normals;          // [B*R][3]
  float* shaded;           // [B*R] or nullptr
};

__global__ void __launch_bounds__(kThreads) shade_normals_kernel(const ShadeParams p) {
  const long long ray = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (ray >= (long long)p.B * p.R) return;
  const long long b = ray / p.R, r = ray - b * p.R;
  const float* gp = p.grads + (b * p.rows_per_image + r) * 3;
  const float gx = gp[0], gy = gp[1], gz = gp[2];
  const float s = __fadd_rn(__fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy)), __fmul_rn(gz, gz));
  const float len = sqrtf(s);          // correctly rounded (clang's default for HIP); __fsqrt_rn maps to the native, approximate square root here
  float n[3] = {0.f, 0.f, 0.f};
  if (!(len == 0.f)) {
    n[0] = __fdiv_rn(-gx, len); n[1] = __fdiv_rn(-gy, len); n[2] = __fdiv_rn(-gz, len);
  }
  float m[3] = {n[0], n[1], n[2]};
  if (p.cam2world) {
    const float* Rm = p.cam2world + b * 9;
    for (int j = 0; j < 3; ++j)
      m[j] = __fadd_rn(__fadd_rn(__fmul_rn(Rm[j], n[0]), __fmul_rn(Rm[3 + j], n[1])), __fmul_rn(Rm[6 + j], n[2]));
  }
  float a = 1.f;
  bool visible = true;
  if (p.alpha) {
    const float raw = p.alpha[ray];
    a = raw;
    if (a < 0.f) a = 0.f;          // ordered compares: NaN stays NaN
    if (a > 1.f) a = 1.f;
    visible = raw >= p.alpha_min;
  }
  const float d = __fadd_rn(__fadd_rn(__fmul_rn(m[0], p.light[0]), __fmul_rn(m[1], p.light[1])), __fmul_rn(m[2], p.light[2]));
  const float lam = d < 0.f ? 0.f : d;          // NaN stays NaN
  const float shade = __fadd_rn(p.ambient, __fmul_rn(__fsub_rn(1.f, p.ambient), lam));
  const float blended = __fadd_rn(__fmul_rn(a, shade), __fmul_rn(__fsub_rn(1.f, a), p.background));
  for (int k = 0; k < 3; ++k) p.normals[ray * 3 + k] = visible ? m[k] : 0.f;
  if (p.shaded) p.shaded[ray] = visible ? blended : p.background;
}

int blocks_for(const char* who, long long rows, unsigned* blocks) {
  const long long b = (rows + kThreads - 1) / kThreads;
  if (b > INT32_MAX) return fail(FENERF_E_INVALID, std::string(who) + ": too many rows for one launch");
  *blocks = (unsigned)b;
  return FENERF_OK;
}

}  // namespace

}  // namespace fenerf

using namespace fenerf;

extern "C" int fenerf_surface_points(int B, int R, const float* origins, const float* dirs, const float* depth, const float* alpha, float alpha_min,
                                     float* points, void* stream) {
  if (B < 0 || R < 0) return fail(FENERF_E_INVALID, "fenerf_surface_points: negative count");
  if (alpha && !(std::isfinite(alpha_min) && alpha_min > 0.f)) return fail(FENERF_E_INVALID, "fenerf_surface_points: alpha_min must be finite and > 0 when alpha is given");
  if ((long long)B * R == 0) return FENERF_OK;
  if (!origins || !dirs || !depth || !points) return fail(FENERF_E_INVALID, "fenerf_surface_points: origins / dirs / depth / points is NULL");
  SurfaceParams p;
  p.B = B; p.R = R; p.Pp = ((long long)R + 31) / 32 * 32;
  p.origins = origins; p.dirs = dirs; p.depth = depth; p.alpha = alpha; p.alpha_min = alpha_min; p.points = points;
  unsigned blocks;
  if (int rc = blocks_for("fenerf_surface_points", (long long)B * p.Pp, &blocks)) return rc;
  PhaseScope ph(PH_OTHER, stream);
  hipLaunchKernelGGL(surface_points_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, p);
  return check_launch("surface points launch");
}

extern "C" int fenerf_volume_sample_grad(const float* vol, int n0, int n1, int n2, int ld, int channel, const float origin[3], const float spacing[3],
                                         int64_t P, const float* points, float* grads, void* stream) {
  const char* who = "fenerf_volume_sample_grad";
  if (n0 < 2 || n1 < 2 || n2 < 2) return fail(FENERF_E_INVALID, std::string(who) + ": every lattice axis needs at least 2 points");
  if ((long long)n0 * n1 > INT32_MAX || (long long)n0 * n1 * n2 > INT32_MAX) return fail(FENERF_E_INVALID, std::string(who) + ": more than 2^31 - 1 lattice points");
  if (!vol || !origin || !spacing) return fail(FENERF_E_INVALID, std::string(who) + ": vol / origin / spacing is NULL");
  if (channel < 0 || channel >= ld) return fail(FENERF_E_INVALID, std::string(who) + ": need 0 <= channel < ld");
  for (int k = 0; k < 3; ++k)
    if (!(std::isfinite(spacing[k]) && spacing[k] > 0.f)) return fail(FENERF_E_INVALID, std::string(who) + ": spacing must be finite and positive");
  if (P < 0) return fail(FENERF_E_INVALID, std::string(who) + ": negative count");
  if (P == 0) return FENERF_OK;
  if (!points || !grads) return fail(FENERF_E_INVALID, std::string(who) + ": points / grads is NULL");
  VolumeGradParams p;
  p.vol = vol; p.n0 = n0; p.n1 = n1; p.n2 = n2; p.ld = ld; p.channel = channel;
  for (int k = 0; k < 3; ++k) { p.origin[k] = origin[k]; p.spacing[k] = spacing[k]; }
  p.P = P; p.points = points; p.grads = grads;
  unsigned blocks;
  if (int rc = blocks_for(who, P, &blocks)) return rc;
  PhaseScope ph(PH_OTHER, stream);
  hipLaunchKernelGGL(volume_sample_grad_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, p);
  return check_launch("volume sample gradient launch");
}

extern "C" int fenerf_shade_normals(int B, int R, int64_t rows_per_image, const float* grads, const float* alpha, const float* cam2world,
                                    const float light[3], float ambient, float background, float alpha_min, float* normals, float* shaded,
                                    void* stream) {
  if (B < 0 || R < 0 || rows_per_image < 0) return fail(FENERF_E_INVALID, "fenerf_shade_normals: negative count");
  if (rows_per_image < R) return fail(FENERF_E_INVALID, "fenerf_shade_normals: rows_per_image < R");
  if (!(std::isfinite(ambient) && std::isfinite(background) && std::isfinite(alpha_min)))
    return fail(FENERF_E_INVALID, "fenerf_shade_normals: ambient / background / alpha_min must be finite");
  if (!grads || !normals || !light) return fail(FENERF_E_INVALID, "fenerf_shade_normals: grads / normals / light is NULL");
  if ((long long)B * R == 0) return FENERF_OK;
  ShadeParams p;
  p.B = B; p.R = R; p.rows_per_image = rows_per_image;
  p.grads = grads; p.alpha = alpha; p.cam2world = cam2world;
  for (int k = 0; k < 3; ++k) p.light[k] = light[k];
  p.ambient = ambient; p.background = background; p.alpha_min = alpha_min;
  p.normals = normals; p.shaded = shaded;
  unsigned blocks;
  if (int rc = blocks_for("fenerf_shade_normals", (long long)B * R, &blocks)) return rc;
  PhaseScope ph(PH_OTHER, stream);
  hipLaunchKernelGGL(shade_normals_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, p);
  return check_launch("shade normals launch");
}
