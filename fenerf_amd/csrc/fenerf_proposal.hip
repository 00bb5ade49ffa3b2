// Proposal depths of a render from a baked density lattice (fenerf_proposal_depths, include/fenerf.h "proposal lattice"): the coarse pass of
// a hierarchical render -- sigma at N stratified depths, the coarse weights, the inverse-CDF resampling -- with the SIREN evaluation replaced
// by a trilinear lookup into vol [n0][n1][n2] fp32, and the N fine depths of every ray left in ascending order for one SIREN pass + composite.
// One wave owns a ray, lane = sample (slot s of lane l is sample 64 s + l, as in fenerf_composite_ray.h):
//   1. sigma at origins + dirs * z: the statement of fenerf_volume_sample_rays for C = 1, ld = 1 (fenerf_volume.hip, rules 1-7 of the header)
//      -- eight scattered dword loads per sample; consecutive lanes are consecutive samples of the ray, so the cells the ray walks
//      through are re-read from L1 / L2 by the wave that fetched them.  sigma goes to LDS, never to memory;
//   2. weights and fine depths: composite_ray<false, .> itself (fenerf_composite_ray.h) on a parameter block whose row, depth and output
//      pointers are this ray's -- rows [N][1] = the sigma in LDS, z_fine = an LDS array.  The arithmetic is not restated here;
//   3. the N fine depths are ranked in the total order of merge_rank (stable ascending, NaN last: torch.sort) and leave LDS in that order.
// No atomics, no workgroup waits for another: the same bytes on every run.
#include <hip/hip_runtime.h>

#include "fenerf_composite_ray.h"
#include "fenerf_internal.h"

namespace fenerf {

namespace {

constexpr int kWaves = 4;      // rays in flight per workgroup; six LDS arrays per wave, 48 KiB per workgroup at 512 samples

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float lerp_rn(float a, float b, float f) {
  return __fadd_rn(__fmul_rn(a, __fsub_rn(1.f, f)), __fmul_rn(b, f));
}

// volume_sample_kernel<1> (fenerf_volume.hip) for one channel of a lattice with ld = 1: the same operations in the same order
__device__ __forceinline__ float lattice_sigma(const ProposalParams& p, const float x[3]) {
  const int n[3] = {p.n0, p.n1, p.n2};
  float t[3];
  bool inside = true;
  for (int k = 0; k < 3; ++k) {
    t[k] = __fdiv_rn(__fsub_rn(x[k], p.origin[k]), p.spacing[k]);
    inside = inside && t[k] >= 0.f && t[k] <= (float)(n[k] - 1);          // ordered: false for NaN
  }
  if (!inside) return p.outside_last;                                     // loads nothing
  int i[3];
  float f[3];
  for (int k = 0; k < 3; ++k) {
    i[k] = min((int)floorf(t[k]), n[k] - 2);
    f[k] = __fsub_rn(t[k], (float)i[k]);
  }
  const long long s1 = p.n2, s0 = (long long)p.n1 * p.n2;
  const float* base = p.vol + (long long)((i[0] * p.n1 + i[1]) * p.n2 + i[2]);      // at most 2^31 - 1 lattice points (checked by the entry)
  float v[8];      // corner d0 d1 d2 at index d0 * 4 + d1 * 2 + d2
  for (int c = 0; c < 8; ++c) v[c] = base[(c >> 2) * s0 + ((c >> 1) & 1) * s1 + (c & 1)];
  const float c00 = lerp_rn(v[0], v[1], f[2]), c01 = lerp_rn(v[2], v[3], f[2]);       // axis 2
  const float c10 = lerp_rn(v[4], v[5], f[2]), c11 = lerp_rn(v[6], v[7], f[2]);
  const float c0 = lerp_rn(c00, c01, f[1]), c1 = lerp_rn(c10, c11, f[1]);              // axis 1
  return lerp_rn(c0, c1, f[0]);                                                       // axis 0
}

template <int MAXM>
__global__ __launch_bounds__(64 * kWaves) void proposal_depths_kernel(const ProposalParams p) {
  constexpr int SLOTS = MAXM / 64;
  __shared__ float s_z[kWaves][MAXM];        // composite_ray: the cdf; then the fine depths by sorted position
  __shared__ float s_zs[kWaves][MAXM + 1];   // composite_ray: the coarse depths
  __shared__ int s_ord[kWaves][MAXM];
  __shared__ float s_w[kWaves][MAXM];        // composite_ray: the coarse weights
  __shared__ float s_sig[kWaves][MAXM];      // sigma of the coarse samples: the ray's rows [N][1]
  __shared__ float s_zf[kWaves][MAXM];       // fine depths by draw index

  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int N = p.N;
  CompositeParams Q{};                       // one ray: composite_ray is called with ray 0 on this ray's pointers
  Q.BR = 1; Q.M = N; Q.C = 1; Q.N = N;
  Q.o.clamp_mode = p.clamp_mode; Q.o.noise_std = p.noise_std;
  Q.sigma_only = 1;
  Q.rows_a = s_sig[wv];
  Q.z_fine = s_zf[wv];
  const long long nwaves = (long long)gridDim.x * kWaves;
  for (long long ray = (long long)blockIdx.x * kWaves + wv; ray < p.BR; ray += nwaves) {
    float o[3], d[3];
    for (int k = 0; k < 3; ++k) { o[k] = p.origins[ray * 3 + k]; d[k] = p.dirs[ray * 3 + k]; }
    const float* z = p.z + ray * N;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int i = lane + 64 * s;
      if (i < N) {
        const float zi = z[i];
        float x[3];
        for (int k = 0; k < 3; ++k) x[k] = __fadd_rn(o[k], __fmul_rn(d[k], zi));
        s_sig[wv][i] = lattice_sigma(p, x);
      }
    }
    wave_lds_sync();
    Q.z_a = z;
    Q.noise = p.noise ? p.noise + ray * N : nullptr;
    Q.u = p.u + ray * N;
    Q.out_weights = p.weights ? p.weights + ray * N : nullptr;
    composite_ray<false, MAXM>(Q, 0, lane, s_z[wv], s_zs[wv], s_ord[wv], s_w[wv]);
    wave_lds_sync();
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int i = lane + 64 * s;
      if (i < N) s_z[wv][merge_rank(s_zf[wv], N, i)] = s_zf[wv][i];       // a permutation of 0 .. N-1 for any bit pattern
    }
    wave_lds_sync();
    float* out = p.z_fine + ray * N;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int i = lane + 64 * s;
      if (i < N) out[i] = s_z[wv][i];
    }
    wave_lds_sync();
  }
}

template <int MAXM>
void launch_for(const ProposalParams& p, void* stream) {
  long long blocks = (p.BR + kWaves - 1) / kWaves;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(proposal_depths_kernel<MAXM>, dim3((unsigned)blocks), dim3(64 * kWaves), 0, (hipStream_t)stream, p);
}

}  // namespace

int launch_proposal_depths(const ProposalParams& p, void* stream) {
  if (p.BR <= 0) return FENERF_OK;
  // the smallest slot count that holds the ray: a skipped slot contributes exact zeros (fenerf_composite_ray.h)
  if (p.N <= 128) launch_for<128>(p, stream);
  else if (p.N <= 256) launch_for<256>(p, stream);
  else launch_for<512>(p, stream);
  return check_launch("proposal depths launch");
}

}  // namespace fenerf
