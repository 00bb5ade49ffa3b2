// Iso-surface extraction on the device (fenerf_mesh_count / fenerf_mesh_emit, include/fenerf.h): marching tetrahedra on the Kuhn
// decomposition of the lattice.  fenerf_amd/mesh_emulation.py restates every step in numpy; tests compare vertices bit for bit.
//   count: classify (7-bit crossing mask of every point's owned edges; faces per cell) -> exclusive scans (per-256 block counts, one
//          workgroup per array with a running int64 carry, per-point add) -> totals
//   emit:  vertex number of owned edge k of point i = prefix[i] + popcount(mask[i] & ((1 << (k - 1)) - 1)); a face looks its three
//          vertex numbers up the same way.  Placement is by prefix sums alone (no atomics): the same bits on every run.
// Addresses and indices are functions of integer indices and of the `>= iso` bits only; a neighbour is read only when it is in the lattice.
#include <hip/hip_runtime.h>

#include "fenerf_internal.h"
#include "fenerf_scan.h"

namespace fenerf {

namespace {

// One tet's crossing edges per sign pattern s (bit v: tet vertex v inside): n = 0 (no face), 3 (a triangle) or 4 (a quad, cyclic);
// e = corner offset of the edge's lower endpoint (bit j: axis j) | k << 3.  Wound so that the normal of the first three points to the
// not-inside side, decided from integer geometry: the doubled edge midpoints stand in for the vertices, the direction from the inside
// vertices' centroid to the other vertices' centroid is the reference (mesh_emulation.tet_case).
struct TetCase { unsigned char n, e[4]; };
struct TetTable { TetCase c[6][16]; };

constexpr int kPerm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

constexpr TetTable make_tet_table() {
  TetTable T{};
  for (int t = 0; t < 6; ++t) {
    int w[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {1, 1, 1}};
    w[1][kPerm[t][0]] = 1;
    w[2][kPerm[t][0]] = 1;
    w[2][kPerm[t][1]] = 1;
    for (int s = 1; s < 15; ++s) {
      int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, nin = 0, nout = 0;
      for (int v = 0; v < 4; ++v) {
        if ((s >> v) & 1) in[nin++] = v;
        else out[nout++] = v;
      }
      int ea[4] = {0, 0, 0, 0}, eb[4] = {0, 0, 0, 0}, n = 3;
      if (nin == 1) {
        for (int j = 0; j < 3; ++j) { ea[j] = in[0]; eb[j] = out[j]; }
      } else if (nout == 1) {
        for (int j = 0; j < 3; ++j) { ea[j] = out[0]; eb[j] = in[j]; }
      } else {
        n = 4;
        ea[0] = in[0]; eb[0] = out[0];
        ea[1] = in[0]; eb[1] = out[1];
        ea[2] = in[1]; eb[2] = out[1];
        ea[3] = in[1]; eb[3] = out[0];
      }
      int m[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, ref[3] = {0, 0, 0};
      for (int j = 0; j < 3; ++j)
        for (int x = 0; x < 3; ++x) m[j][x] = w[ea[j]][x] + w[eb[j]][x];
      for (int x = 0; x < 3; ++x) {
        int so = 0, si = 0;
        for (int j = 0; j < nout; ++j) so += w[out[j]][x];
        for (int j = 0; j < nin; ++j) si += w[in[j]][x];
        ref[x] = nin * so - nout * si;
      }
      const int u[3] = {m[1][0] - m[0][0], m[1][1] - m[0][1], m[1][2] - m[0][2]};
      const int v[3] = {m[2][0] - m[0][0], m[2][1] - m[0][1], m[2][2] - m[0][2]};
      const int dot = (u[1] * v[2] - u[2] * v[1]) * ref[0] + (u[2] * v[0] - u[0] * v[2]) * ref[1] + (u[0] * v[1] - u[1] * v[0]) * ref[2];
      if (dot < 0) {      // reverse the cycle, keeping its first edge
        const int a1 = ea[1], b1 = eb[1];
        ea[1] = ea[n - 1]; eb[1] = eb[n - 1];
        ea[n - 1] = a1; eb[n - 1] = b1;
      }
      T.c[t][s].n = (unsigned char)n;
      for (int j = 0; j < n; ++j) {
        const int lo = ea[j] < eb[j] ? ea[j] : eb[j], hi = ea[j] < eb[j] ? eb[j] : ea[j];
        const int corner = w[lo][0] | w[lo][1] << 1 | w[lo][2] << 2;
        const int k = (w[hi][0] - w[lo][0]) | (w[hi][1] - w[lo][1]) << 1 | (w[hi][2] - w[lo][2]) << 2;
        T.c[t][s].e[j] = (unsigned char)(corner | k << 3);
      }
    }
  }
  return T;
}

__device__ const TetTable kTet = make_tet_table();

struct Lattice {
  int n0, n1, n2;
  long long n, cells;      // points, cells
};

// the `inside` bits of a cell's eight corners (bit o: corner offset o, bit j of o = axis j); i = linear index of the cell's corner c
__device__ __forceinline__ int corner_bits(const float* __restrict__ vol, const Lattice L, long long i, float iso) {
  const long long s0 = (long long)L.n1 * L.n2, s1 = L.n2;
  int bits = 0;
#pragma unroll
  for (int o = 0; o < 8; ++o) bits |= (vol[i + (o & 1) * s0 + ((o >> 1) & 1) * s1 + (o >> 2)] >= iso ? 1 : 0) << o;
  return bits;
}

// sign pattern of tet t of a cell from its corner bits
__device__ __forceinline__ int tet_pattern(int bits, int t) {
  const int c1 = 1 << kPerm[t][0], c2 = c1 | 1 << kPerm[t][1];
  return (bits & 1) | ((bits >> c1) & 1) << 1 | ((bits >> c2) & 1) << 2 | ((bits >> 7) & 1) << 3;
}

// One lane per lattice point: the crossing mask of its owned edges, and the workgroup's count of crossing edges.
__global__ void __launch_bounds__(256) mesh_classify_points_kernel(const float* __restrict__ vol, const Lattice L, float iso, unsigned char* __restrict__ mask,
                                                                   int* __restrict__ block_counts) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  int m = 0;
  if (i < L.n) {
    const int c = (int)(i % L.n2), b = (int)((i / L.n2) % L.n1), a = (int)(i / ((long long)L.n1 * L.n2));
    const bool in_p = vol[i] >= iso;
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      const int d0 = k & 1, d1 = (k >> 1) & 1, d2 = k >> 2;
      if (a + d0 < L.n0 && b + d1 < L.n1 && c + d2 < L.n2) {
        const bool in_q = vol[i + d0 * (long long)L.n1 * L.n2 + d1 * (long long)L.n2 + d2] >= iso;
        m |= (in_q != in_p ? 1 : 0) << (k - 1);
      }
    }
    mask[i] = (unsigned char)m;
  }
  int total;
  block_scan_256(__popc(m), &total);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

// One lane per cell: its face count (0 .. 12), and the workgroup's count of faces.
__global__ void __launch_bounds__(256) mesh_classify_cells_kernel(const float* __restrict__ vol, const Lattice L, float iso, unsigned char* __restrict__ nfaces,
                                                                  int* __restrict__ block_counts) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  int f = 0;
  if (j < L.cells) {
    const int m1 = L.n1 - 1, m2 = L.n2 - 1;
    const long long a = j / ((long long)m1 * m2), b = (j / m2) % m1, c = j % m2;
    const int bits = corner_bits(vol, L, (a * L.n1 + b) * L.n2 + c, iso);
    if (bits != 0 && bits != 255) {
#pragma unroll
      for (int t = 0; t < 6; ++t) {
        const int pc = __popc(tet_pattern(bits, t));
        f += pc == 2 ? 2 : (pc == 1 || pc == 3 ? 1 : 0);
      }
    }
    nfaces[j] = (unsigned char)f;
  }
  int total;
  block_scan_256(f, &total);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

// One lane per lattice point: prefix[i] = crossing edges of all points before i
__global__ void __launch_bounds__(256) mesh_point_prefix_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ block_prefix, long long n,
                                                                int* __restrict__ prefix) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  int total;
  const int before = block_scan_256(i < n ? __popc((int)mask[i]) : 0, &total);
  if (i < n) prefix[i] = block_prefix[blockIdx.x] + before;
}

struct Frame { float origin[3], spacing[3]; };

// One lane per lattice point: the vertices of its crossing owned edges, in ascending k, from slot prefix[i]
__global__ void __launch_bounds__(256) mesh_emit_vertices_kernel(const float* __restrict__ vol, const Lattice L, float iso, const Frame fr,
                                                                 const unsigned char* __restrict__ mask, const int* __restrict__ prefix, long long n_vertices,
                                                                 float* __restrict__ vertices) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= L.n) return;
  const int m = mask[i];
  if (m == 0) return;
  const int p[3] = {(int)(i / ((long long)L.n1 * L.n2)), (int)((i / L.n2) % L.n1), (int)(i % L.n2)};
  const float vp = vol[i];
  const long long first = prefix[i];
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    if (!((m >> (k - 1)) & 1)) continue;
    const int d[3] = {k & 1, (k >> 1) & 1, k >> 2};
    const long long slot = first + __popc(m & ((1 << (k - 1)) - 1));
    if (slot >= n_vertices) continue;
    // bit k - 1 of the mask says that p + d_k is in the lattice
    const float vq = vol[i + d[0] * (long long)L.n1 * L.n2 + d[1] * (long long)L.n2 + d[2]];
    const float t = __fsub_rn(iso, vp) / __fsub_rn(vq, vp);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float x = __fadd_rn(fr.origin[j], __fmul_rn(__fadd_rn((float)p[j], __fmul_rn(t, (float)d[j])), fr.spacing[j]));
      __builtin_nontemporal_store(x, vertices + slot * 3 + j);
    }
  }
}

// One lane per cell: its faces, tet by tet, from the slot its workgroup's prefix and the scan of the workgroup's face counts give
__global__ void __launch_bounds__(256) mesh_emit_faces_kernel(const float* __restrict__ vol, const Lattice L, float iso, const unsigned char* __restrict__ mask,
                                                              const int* __restrict__ prefix, const unsigned char* __restrict__ nfaces,
                                                              const int* __restrict__ block_prefix, long long n_vertices, long long n_faces,
                                                              int* __restrict__ faces) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  const int f = j < L.cells ? nfaces[j] : 0;
  int total;
  long long slot = (long long)block_prefix[blockIdx.x] + block_scan_256(f, &total);
  if (f == 0) return;
  const int m1 = L.n1 - 1, m2 = L.n2 - 1;
  const long long a = j / ((long long)m1 * m2), b = (j / m2) % m1, c = j % m2;
  const long long i = (a * L.n1 + b) * L.n2 + c;
  const int bits = corner_bits(vol, L, i, iso);
  for (int t = 0; t < 6; ++t) {
    const TetCase tc = kTet.c[t][tet_pattern(bits, t)];
    if (tc.n == 0) continue;
    int vn[4] = {0, 0, 0, 0};
    for (int e = 0; e < tc.n; ++e) {
      const int corner = tc.e[e] & 7, k = tc.e[e] >> 3;
      const long long ip = i + (corner & 1) * (long long)L.n1 * L.n2 + ((corner >> 1) & 1) * (long long)L.n2 + (corner >> 2);
      vn[e] = prefix[ip] + __popc((int)mask[ip] & ((1 << (k - 1)) - 1));
    }
    int q = 0;      // a quad is split along the diagonal through its smallest vertex number
    if (tc.n == 4) {
      for (int e = 1; e < 4; ++e) q = vn[e] < vn[q] ? e : q;
    }
    for (int tri = 0; tri < tc.n - 2; ++tri, ++slot) {
      if (slot >= n_faces) continue;
      const int v0 = vn[q], v1 = vn[(q + 1 + tri) & 3], v2 = vn[(q + 2 + tri) & 3];
      __builtin_nontemporal_store(v0, faces + slot * 3 + 0);
      __builtin_nontemporal_store(v1, faces + slot * 3 + 1);
      __builtin_nontemporal_store(v2, faces + slot * 3 + 2);
    }
  }
}

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// workspace: totals int64 [2] | prefix int32 [n] | point block counts int32 | cell block counts int32 | mask uint8 [n] | faces per cell uint8
struct MeshWs {
  long long n, cells, nblk_v, nblk_f;
  size_t totals, prefix, blocks_v, blocks_f, mask, nfaces, bytes;
};
MeshWs mesh_ws(int n0, int n1, int n2) {
  MeshWs w;
  w.n = (long long)n0 * n1 * n2;
  w.cells = (long long)(n0 - 1) * (n1 - 1) * (n2 - 1);
  w.nblk_v = (w.n + 255) / 256;
  w.nblk_f = (w.cells + 255) / 256;
  size_t off = 0;
  w.totals = off; off += 256;
  w.prefix = off; off += up256((size_t)w.n * sizeof(int));
  w.blocks_v = off; off += up256((size_t)w.nblk_v * sizeof(int));
  w.blocks_f = off; off += up256((size_t)w.nblk_f * sizeof(int));
  w.mask = off; off += up256((size_t)w.n);
  w.nfaces = off; off += up256((size_t)w.cells);
  w.bytes = off;
  return w;
}

}  // namespace

size_t mesh_workspace_bytes(int n0, int n1, int n2) { return mesh_ws(n0, n1, n2).bytes; }

// the two totals fenerf_mesh_count left in the workspace (its first 16 bytes, whatever the lattice)
const long long* mesh_workspace_totals(const void* workspace) { return (const long long*)workspace; }

int launch_mesh_count(const float* vol, int n0, int n1, int n2, float iso, void* workspace, long long* counts_dev, void* stream) {
  const MeshWs w = mesh_ws(n0, n1, n2);
  char* ws = (char*)workspace;
  const Lattice L = {n0, n1, n2, w.n, w.cells};
  int* blocks_v = (int*)(ws + w.blocks_v);
  int* blocks_f = (int*)(ws + w.blocks_f);
  unsigned char* mask = (unsigned char*)(ws + w.mask);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mesh_classify_points_kernel, dim3((unsigned)w.nblk_v), dim3(256), 0, s, vol, L, iso, mask, blocks_v);
  hipLaunchKernelGGL(mesh_classify_cells_kernel, dim3((unsigned)w.nblk_f), dim3(256), 0, s, vol, L, iso, (unsigned char*)(ws + w.nfaces), blocks_f);
  hipLaunchKernelGGL(block_counts_scan_kernel, dim3(2), dim3(1024), 0, s, blocks_v, w.nblk_v, blocks_f, w.nblk_f, (long long*)(ws + w.totals), counts_dev);
  hipLaunchKernelGGL(mesh_point_prefix_kernel, dim3((unsigned)w.nblk_v), dim3(256), 0, s, mask, blocks_v, w.n, (int*)(ws + w.prefix));
  return check_launch("mesh count launch");
}

int launch_mesh_emit(const float* vol, int n0, int n1, int n2, float iso, const float* origin, const float* spacing, const void* workspace,
                     long long n_vertices, long long n_faces, float* vertices, int* faces, void* stream) {
  const MeshWs w = mesh_ws(n0, n1, n2);
  const char* ws = (const char*)workspace;
  const Lattice L = {n0, n1, n2, w.n, w.cells};
  const unsigned char* mask = (const unsigned char*)(ws + w.mask);
  const int* prefix = (const int*)(ws + w.prefix);
  hipStream_t s = (hipStream_t)stream;
  if (n_vertices > 0) {
    const Frame fr = {{origin[0], origin[1], origin[2]}, {spacing[0], spacing[1], spacing[2]}};
    hipLaunchKernelGGL(mesh_emit_vertices_kernel, dim3((unsigned)w.nblk_v), dim3(256), 0, s, vol, L, iso, fr, mask, prefix, n_vertices, vertices);
  }
  if (n_faces > 0)
    hipLaunchKernelGGL(mesh_emit_faces_kernel, dim3((unsigned)w.nblk_f), dim3(256), 0, s, vol, L, iso, mask, prefix, (const unsigned char*)(ws + w.nfaces),
                       (const int*)(ws + w.blocks_f), n_vertices, n_faces, faces);
  return check_launch("mesh emit launch");
}

}  // namespace fenerf
