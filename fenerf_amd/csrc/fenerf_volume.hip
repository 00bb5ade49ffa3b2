// Trilinear sampling of a channels-last lattice (fenerf_volume_sample / fenerf_volume_sample_rays, include/fenerf.h "baked radiance
// lattice"): vol [n0][n1][n2][ld] fp32, C <= ld channels per lattice point, rows [P][C] out.  fenerf_amd/volume_emulation.py restates the
// arithmetic in numpy; tests compare bit for bit.
// One wave owns 64 consecutive samples (consecutive samples of a ray, so the cells a ray walks through are re-read from L1 / L2 by the
// wave that fetched them):
//   1. lane = sample: position (given, or origins + dirs * z), t = (p - origin) / spacing, the inside test, the clamped cell index and
//      the three fractions -> 16 bytes of LDS per sample;
//   2. lane = (sample, piece): the 64 x Q pieces of the wave's rows are dealt to the lanes in row-major order, so that consecutive lanes
//      read consecutive pieces of a corner row -- 16-byte pieces (global_load_dwordx4; ld % 4 == 0 and a 16-byte-aligned base) or
//      dwords (any ld).  Eight corner loads and seven lerps per channel, the same operations in both forms: the same bits;
//   3. the wave's 64 rows are contiguous in `rows`: they leave LDS as 256 contiguous bytes per store instruction.
// Addresses come from the clamped integer cell index alone; a point that fails the (ordered) inside test loads nothing.  No atomics, no
// workgroup waits for another: the same bytes on every run.
#include <hip/hip_runtime.h>

#include "fenerf_internal.h"

namespace fenerf {

namespace {

constexpr int kMaxWaves = 4;    // per workgroup; every wave works on its own 64 samples

__device__ __forceinline__ float lerp_rn(float a, float b, float f) {
  return __fadd_rn(__fmul_rn(a, __fsub_rn(1.f, f)), __fmul_rn(b, f));
}

// W = 4: a piece is a float4 (piece q = channels 4 q .. 4 q + 3, all inside the ld floats of the lattice point); W = 1: a dword
template <int W>
__global__ void __launch_bounds__(64 * kMaxWaves) volume_sample_kernel(const VolumeParams p) {
  extern __shared__ int4 volume_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  const int C = p.C;
  int4* meta = volume_lds + wave * 64;                                            // [waves][64]: cell (-1 outside), f0, f1, f2
  float* tile = reinterpret_cast<float*>(volume_lds + waves * 64) + (size_t)wave * 64 * C;      // [waves][64][C]
  const long long first = ((long long)blockIdx.x * waves + wave) * 64;
  const long long left = p.P - first;
  const int count = left >= 64 ? 64 : (left > 0 ? (int)left : 0);                  // samples of this wave

  int cell = -1;
  float f[3] = {0.f, 0.f, 0.f};
  if (lane < count) {
    const long long s = first + lane;
    float x[3];
    if (p.points) {
      for (int k = 0; k < 3; ++k) x[k] = p.points[s * 3 + k];
    } else {
      const long long ray = s / p.N;
      const float z = p.z[s];
      for (int k = 0; k < 3; ++k) x[k] = __fadd_rn(p.origins[ray * 3 + k], __fmul_rn(p.dirs[ray * 3 + k], z));
    }
    const int n[3] = {p.n0, p.n1, p.n2};
    float t[3];
    bool inside = true;
    for (int k = 0; k < 3; ++k) {
      t[k] = __fdiv_rn(__fsub_rn(x[k], p.origin[k]), p.spacing[k]);
      inside = inside && t[k] >= 0.f && t[k] <= (float)(n[k] - 1);          // ordered: false for NaN
    }
    if (inside) {
      int i[3];
      for (int k = 0; k < 3; ++k) {
        i[k] = min((int)floorf(t[k]), n[k] - 2);
        f[k] = __fsub_rn(t[k], (float)i[k]);
      }
      cell = (i[0] * p.n1 + i[1]) * p.n2 + i[2];
    }
  }
  meta[lane] = make_int4(cell, __float_as_int(f[0]), __float_as_int(f[1]), __float_as_int(f[2]));
  __syncthreads();

  const int Q = (C + W - 1) / W;
  const long long s2 = p.ld, s1 = (long long)p.n2 * p.ld, s0 = (long long)p.n1 * s1;       // strides in floats
  for (int e = lane; e < count * Q; e += 64) {
    const int s = e / Q, q = e - s * Q;
    const int4 m = meta[s];
    float r[W];
    if (m.x < 0) {
      for (int j = 0; j < W; ++j) r[j] = q * W + j == C - 1 ? p.outside_last : 0.f;
    } else {
      const float f0 = __int_as_float(m.y), f1 = __int_as_float(m.z), f2 = __int_as_float(m.w);
      const float* base = p.vol + (long long)m.x * p.ld + q * W;
      float v[8][W];      // corner d0 d1 d2 at index d0 * 4 + d1 * 2 + d2
      for (int c = 0; c < 8; ++c) {
        const float* src = base + (c >> 2) * s0 + ((c >> 1) & 1) * s1 + (c & 1) * s2;
        if constexpr (W == 4) {
          const float4 a = *reinterpret_cast<const float4*>(src);
          v[c][0] = a.x; v[c][1] = a.y; v[c][2] = a.z; v[c][3] = a.w;
        } else {
          v[c][0] = *src;
        }
      }
      for (int j = 0; j < W; ++j) {
        const float c00 = lerp_rn(v[0][j], v[1][j], f2), c01 = lerp_rn(v[2][j], v[3][j], f2);       // axis 2
        const float c10 = lerp_rn(v[4][j], v[5][j], f2), c11 = lerp_rn(v[6][j], v[7][j], f2);
        const float c0 = lerp_rn(c00, c01, f1), c1 = lerp_rn(c10, c11, f1);                          // axis 1
        r[j] = lerp_rn(c0, c1, f0);                                                                 // axis 0
      }
    }
    for (int j = 0; j < W; ++j)
      if (q * W + j < C) tile[s * C + q * W + j] = r[j];
  }
  __syncthreads();

  float* out = p.rows + first * C;
  for (int i = lane; i < count * C; i += 64) out[i] = tile[i];
}

}  // namespace

int launch_volume_sample(const VolumeParams& p, void* stream) {
  const int waves = p.C <= 32 ? kMaxWaves : 2;          // LDS per workgroup: 64 (16 + 4 C) bytes per wave, 36,864 B at most
  const long long blocks = (p.P + 64 * waves - 1) / (64 * waves);
  if (blocks > INT32_MAX) return fail(FENERF_E_INVALID, "volume sample: too many points for one launch");
  const size_t lds = (size_t)waves * 64 * (sizeof(int4) + (size_t)p.C * sizeof(float));
  const bool x4 = p.ld % 4 == 0 && ((uintptr_t)p.vol & 15) == 0;
  if (x4) hipLaunchKernelGGL(volume_sample_kernel<4>, dim3((unsigned)blocks), dim3(64 * waves), lds, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(volume_sample_kernel<1>, dim3((unsigned)blocks), dim3(64 * waves), lds, (hipStream_t)stream, p);
  return check_launch("volume sample launch");
}

}  // namespace fenerf
