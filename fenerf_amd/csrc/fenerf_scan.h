// Prefix sums for placement by counting (fenerf_mesh.hip, fenerf_mesh_clean.hip): a 256-thread workgroup scan, and the one-workgroup scan
// of per-workgroup counts with a running int64 carry.  Integer sums only: the same bits on every run.
#pragma once
#include <hip/hip_runtime.h>

namespace fenerf {

namespace {

// exclusive prefix of v over the workgroup's 256 threads; *total = their sum.  Every thread of the workgroup calls it.
__device__ __forceinline__ int block_scan_256(int v, int* total) {
  __shared__ int wave_total[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int incl = v;
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o);
    if (lane >= o) incl += u;
  }
  if (lane == 63) wave_total[w] = incl;
  __syncthreads();
  int before = 0, all = 0;
  for (int k = 0; k < 4; ++k) {
    const int s = wave_total[k];
    if (k < w) before += s;
    all += s;
  }
  __syncthreads();
  *total = all;
  return before + incl - v;
}

// Workgroup 0 / 1: the block counts of array a / of array b become their exclusive prefix sums in place, with a running int64 carry over
// pieces of 1024 blocks; totals[blockIdx.x] (the workspace's copy) and counts_dev[blockIdx.x] (the caller's) = the sum.  A prefix is kept
// as int32: it is only used when the total is below 2^31 (the emit calls refuse anything else).
__global__ void __launch_bounds__(1024) block_counts_scan_kernel(int* __restrict__ counts_a, long long nblk_a, int* __restrict__ counts_b, long long nblk_b,
                                                                 long long* __restrict__ totals, long long* __restrict__ counts_dev) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  int* bc = blockIdx.x == 0 ? counts_a : counts_b;
  const long long nblk = blockIdx.x == 0 ? nblk_a : nblk_b;
  __shared__ long long wave_sum[16];
  __shared__ long long carry_s;
  if (t == 0) carry_s = 0;
  __syncthreads();
  for (long long base = 0; base < nblk; base += 1024) {
    const long long j = base + t;
    const long long v = j < nblk ? bc[j] : 0;
    long long incl = v;
    for (int o = 1; o < 64; o <<= 1) {
      const long long u = __shfl_up(incl, o);
      if (lane >= o) incl += u;
    }
    if (lane == 63) wave_sum[w] = incl;
    __syncthreads();
    long long before = carry_s;
    for (int k = 0; k < w; ++k) before += wave_sum[k];
    if (j < nblk) bc[j] = (int)(before + incl - v);
    __syncthreads();
    if (t == 1023) carry_s = before + incl;
    __syncthreads();
  }
  if (t == 0) {
    totals[blockIdx.x] = carry_s;
    counts_dev[blockIdx.x] = carry_s;
  }
}

}  // namespace

}  // namespace fenerf
