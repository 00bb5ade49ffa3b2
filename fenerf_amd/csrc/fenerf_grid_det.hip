// Deterministic gradient wrt the 3-D feature grid (fenerf_grid_backward_det, and fenerf_render_backward in
// FENERF_GRID_GRAD_DETERMINISTIC mode): the transpose of sample_from_3dgrid (siren.py:314-330) summed in exact integer arithmetic,
// so that the result does not depend on the order of the adds (Guideline 12 of the CDNA HIP guide: float atomics do).
//
// Over ALL rows of a backward pass at once:
//   1. max pass     m = max |d_e| over the finite values; e = its binary exponent (m < 2^e); k = 62 - e - h, h = ceil(log2(dense_rows))
//   2. scatter      per finite non-zero value g and in-bounds corner: q = rint(double(g * (wx * wy * wz)) * 2^k) added as int64
//                   (|q| <= 2^(62 - h) and at most dense_rows >= rows adds per voxel-channel: the sum cannot overflow)
//   3. finish       float(double(acc) * 2^-k), straight into the channels-last or the parameter's NCDHW layout
//   4. non-finite   channel c of every in-bounds corner of a non-finite value is set to NaN (plain stores; skipped when there is none)
// The scale is read from device memory by the kernels: the host never waits.  The trilinear arithmetic is grid_backward_kernel's
// (fenerf_siren_bwd.hip) with FP contraction off, so that a numpy float32 / int64 emulation reproduces the result bit for bit
// (fenerf_amd/grid_det_emulation.py).
#include <hip/hip_runtime.h>

#include "fenerf_grid.h"
#include "fenerf_internal.h"

#pragma clang fp contract(off)

namespace fenerf {

namespace {

struct DetHeader { unsigned int max_bits; unsigned int nonfinite; };
constexpr size_t kHeaderBytes = 256;

__device__ __forceinline__ bool finite_bits(unsigned int b) { return (b & 0x7f800000u) != 0x7f800000u; }

// -k where the scale is 2^k: e from the finite max (m < 2^e; frexp(0) = 0), h from the caller's dense row count
__device__ __forceinline__ int det_shift(const DetHeader* hdr, int h) {
  int e = 0;
  (void)frexpf(__uint_as_float(hdr->max_bits), &e);
  return 62 - e - h;
}

__global__ __launch_bounds__(256) void det_max_kernel(long long n, const float* d_e, DetHeader* hdr) {
  unsigned int mx = 0, bad = 0;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const unsigned int b = __float_as_uint(d_e[i]) & 0x7fffffffu;
    if (finite_bits(b)) mx = b > mx ? b : mx;       // |x| of non-negative floats orders like its bit pattern
    else bad = 1;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned int v = (unsigned int)__shfl_xor((int)mx, o);
    mx = v > mx ? v : mx;
    bad |= (unsigned int)__shfl_xor((int)bad, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (mx) atomicMax(&hdr->max_bits, mx);
    if (bad) atomicOr(&hdr->nonfinite, 1u);
  }
}

// the grid cell of a point: UniformBoxWarp, then fenerf_grid.h
__device__ __forceinline__ GridCell cell_of(const float* p, float box_scale, int gd, int gh, int gw) {
  return grid_cell(p[0] * box_scale, p[1] * box_scale, p[2] * box_scale, gd, gh, gw);
}

// one thread per (row, channel): the 32 lanes of a row add into one voxel's 256-B line of int64 sums per corner
__global__ __launch_bounds__(256) void det_scatter_kernel(long long rows, const float* points, const float* d_e, float box_scale, int gd,
                                                           int gh, int gw, int h, const DetHeader* hdr, unsigned long long* acc) {
  const double scale = ldexp(1.0, det_shift(hdr, h));
  const long long total = rows * 32;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const float g = d_e[i];
    if (g == 0.f || !finite_bits(__float_as_uint(g))) continue;      // zero rows add nothing; non-finite values: pass 4
    const long long pt = i >> 5;
    const int ch = (int)(i & 31);
    const GridCell k = cell_of(points + pt * 3, box_scale, gd, gh, gw);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const GridCorner n = grid_corner(k, c);
      if (n.ok) {
        const float v = g * (n.wx * n.wy * n.wz);
        const long long q = (long long)rint((double)v * scale);
        if (q != 0) atomicAdd(acc + grid_voxel(k, n) * 32 + ch, (unsigned long long)q);     // two's complement: the signed sum
      }
    }
  }
}

// int64 sums -> fp32 gradient.  TO_NCDHW: through an LDS tile of 64 voxels x 32 channels (grid_transpose_kernel's scheme), else in place order.
template <bool TO_NCDHW>
__global__ __launch_bounds__(256) void det_finish_kernel(const long long* acc, float* out, long long vox, int h, const DetHeader* hdr) {
  const double inv = ldexp(1.0, -det_shift(hdr, h));
  const long long v0 = (long long)blockIdx.x * 64;
  const int tid = threadIdx.x;
  if (!TO_NCDHW) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const long long j = v0 * 32 + k * 256 + tid;
      if (j < vox * 32) out[j] = (float)((double)acc[j] * inv);
    }
    return;
  }
  __shared__ float tile[64][33];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int idx = k * 256 + tid, v = idx >> 5, c = idx & 31;
    if (v0 + v < vox) tile[v][c] = (float)((double)acc[(v0 + v) * 32 + c] * inv);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int idx = k * 256 + tid, c = idx >> 6, v = idx & 63;
    if (v0 + v < vox) out[(long long)c * vox + v0 + v] = tile[v][c];
  }
}

template <bool TO_NCDHW>
__global__ __launch_bounds__(256) void det_nonfinite_kernel(long long rows, const float* points, const float* d_e, float box_scale, int gd, int gh,
                                                             int gw, const DetHeader* hdr, float* out) {
  if (!hdr->nonfinite) return;
  const long long total = rows * 32, vox_n = (long long)gd * gh * gw;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    if (finite_bits(__float_as_uint(d_e[i]))) continue;
    const long long pt = i >> 5;
    const int ch = (int)(i & 31);
    const GridCell k = cell_of(points + pt * 3, box_scale, gd, gh, gw);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const GridCorner n = grid_corner(k, c);
      if (n.ok) {
        const long long vox = grid_voxel(k, n);
        out[TO_NCDHW ? (long long)ch * vox_n + vox : vox * 32 + ch] = __builtin_nanf("");
      }
    }
  }
}
}  // namespace

size_t grid_det_workspace_bytes(const FenerfModel* m) {
  if (!m || !m->grid_ch) return 0;
  return kHeaderBytes + (size_t)m->gd * m->gh * m->gw * 32 * sizeof(long long);
}

int launch_grid_backward_det(const FenerfModel* m, long long rows, long long dense_rows, const float* points, const float* d_e, float* out,
                             bool to_ncdhw, void* workspace, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const size_t ws = grid_det_workspace_bytes(m);
  hipError_t e = hipMemsetAsync(workspace, 0, ws, st);
  if (e != hipSuccess) return hip_fail(e, "grid_backward_det: workspace clear");
  int h = 0;
  while (h < 63 && (1LL << h) < dense_rows) ++h;
  DetHeader* hdr = (DetHeader*)workspace;
  unsigned long long* acc = (unsigned long long*)((char*)workspace + kHeaderBytes);
  const long long vox = (long long)m->gd * m->gh * m->gw;
  if (rows > 0) {
    const long long n = rows * 32;
    const unsigned blocks = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(det_max_kernel, dim3(blocks), dim3(256), 0, st, n, d_e, hdr);
    const unsigned sblocks = (unsigned)((n + 255) / 256 < 65536 ? (n + 255) / 256 : 65536);
    hipLaunchKernelGGL(det_scatter_kernel, dim3(sblocks), dim3(256), 0, st, rows, points, d_e, m->box_scale, m->gd, m->gh, m->gw, h, hdr, acc);
  }
  const unsigned fblocks = (unsigned)((vox + 63) / 64);
  if (to_ncdhw) hipLaunchKernelGGL(det_finish_kernel<true>, dim3(fblocks), dim3(256), 0, st, (const long long*)acc, out, vox, h, hdr);
  else hipLaunchKernelGGL(det_finish_kernel<false>, dim3(fblocks), dim3(256), 0, st, (const long long*)acc, out, vox, h, hdr);
  if (rows > 0) {
    const long long n = rows * 32;
    const unsigned blocks = (unsigned)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    if (to_ncdhw) hipLaunchKernelGGL(det_nonfinite_kernel<true>, dim3(blocks), dim3(256), 0, st, rows, points, d_e, m->box_scale, m->gd, m->gh, m->gw, hdr, out);
    else hipLaunchKernelGGL(det_nonfinite_kernel<false>, dim3(blocks), dim3(256), 0, st, rows, points, d_e, m->box_scale, m->gd, m->gh, m->gw, hdr, out);
  }
  return check_launch("grid_backward_det launch");
}

}  // namespace fenerf
