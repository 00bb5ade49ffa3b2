// Cleaning an extracted mesh on the device (include/fenerf.h, "mesh cleaning"): connected components of the inside set of a lattice
// (fenerf_volume_components / fenerf_volume_keep_components) and vertex clustering (fenerf_mesh_cluster_count / _emit).
// fenerf_amd/mesh_emulation.py restates both in numpy; tests compare labels and faces as integers, volumes and vertices bit for bit.
//   components: a union-find forest kept in the labels array itself, parent[i] <= i at every moment.  One kernel joins the two ends of every
//               owned edge (the 7 directions d_k of fenerf_mesh.hip: a 14-neighbourhood) whose ends are both inside, with atomicMin; the
//               next replaces every parent by its root and counts the points of every root.  The root of a tree is its smallest index, so
//               the labels do not depend on the order in which the joins arrive.  No workgroup waits for another.
//   clustering: cluster id of a vertex from its lattice coordinate; the representative is the mean of the members in 2^-16 lattice units,
//               summed as int64 (integer atomicAdd: any order, the same sum).  Placement is by prefix sums (fenerf_scan.h).
// Atomics are integer atomicMin / atomicAdd on global memory; parents are read with relaxed device-scope atomic loads, so that a walk sees
// what the atomics wrote and not a line a compute unit cached before.
#include <hip/hip_runtime.h>

#include "fenerf_internal.h"
#include "fenerf_scan.h"

namespace fenerf {

namespace {

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// ---- connected components ----------------------------------------------------------------------------------------------------------

struct Lattice {
  int n0, n1, n2;
  long long n;
};

__device__ __forceinline__ int parent_of(const int* parent, int i) { return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of i's tree.  Terminates: parent[l] <= l always (a parent is only ever lowered, by atomicMin, and starts at l), so every step of
// the walk strictly lowers l, and it stops at an l that is its own parent.
__device__ __forceinline__ int cc_find(const int* parent, int i) {
  int l = i;
  for (;;) {
    const int p = parent_of(parent, l);
    if (p == l) return l;
    l = p;      // p < l
  }
}

// joins the trees of a and b: the larger root goes under the smaller one.  Terminates: a retry happens only when atomicMin found that the
// larger root a had meanwhile been put under old < a; then old and b are what is left to join (a reaches both), so the larger of the pair
// strictly falls with every retry and the pair is bounded below by 0.
__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
  for (;;) {
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(parent + a, b);       // b < a
    if (old == a) return;
    a = old;                                        // old < a
  }
}

__global__ void __launch_bounds__(256) cc_init_kernel(const float* __restrict__ vol, long long n, float iso, int* __restrict__ labels, int* __restrict__ counts) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  labels[i] = vol[i] >= iso ? (int)i : -1;
  counts[i] = 0;
}

// One lane per lattice point: joins it to the far end of each of its owned edges when both ends are inside.
__global__ void __launch_bounds__(256) cc_join_kernel(const float* __restrict__ vol, const Lattice L, float iso, int* __restrict__ labels) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= L.n) return;
  if (!(vol[i] >= iso)) return;
  const int c = (int)(i % L.n2), b = (int)((i / L.n2) % L.n1), a = (int)(i / ((long long)L.n1 * L.n2));
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    const int d0 = k & 1, d1 = (k >> 1) & 1, d2 = k >> 2;
    if (a + d0 < L.n0 && b + d1 < L.n1 && c + d2 < L.n2) {
      const long long q = i + d0 * (long long)L.n1 * L.n2 + d1 * (long long)L.n2 + d2;
      if (vol[q] >= iso) cc_union(labels, (int)i, (int)q);
    }
  }
}

// After every join: a label becomes its root, and the root's point count takes the point in.  A workgroup walks kFlattenItems x 256 points.
// The first root a wave meets in each 64 points is summed over the workgroup in LDS before it goes to memory -- in a large component that
// is the one root of nearly every wave, and one atomicAdd per wave on its single address was this kernel's whole time; any further root
// of the same 64 points costs one atomicAdd of its own.
constexpr int kFlattenItems = 4;
__global__ void __launch_bounds__(256) cc_flatten_count_kernel(long long n, int* __restrict__ labels, int* __restrict__ counts) {
  __shared__ int s_root[kFlattenItems * 4], s_count[kFlattenItems * 4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int j = 0; j < kFlattenItems; ++j) {
    const long long i = ((long long)blockIdx.x * kFlattenItems + j) * 256 + threadIdx.x;
    int r = -1;
    if (i < n && parent_of(labels, (int)i) >= 0) {
      r = cc_find(labels, (int)i);
      labels[i] = r;      // r <= the parent it replaces: other walks through i still descend
    }
    unsigned long long todo = __ballot(r >= 0);
    int first_root = -1, first_count = 0;      // the same in every lane
    while (todo) {      // terminates: the leader's own bit is in `same`, so the set strictly shrinks
      const int leader = __ffsll((long long)todo) - 1;
      const int lr = __shfl(r, leader);
      const unsigned long long same = __ballot(r == lr) & todo;
      if (first_root < 0) {
        first_root = lr;
        first_count = __popcll(same);
      } else if (lane == leader) {
        atomicAdd(counts + lr, __popcll(same));
      }
      todo &= ~same;
    }
    if (lane == 0) {
      s_root[j * 4 + w] = first_root;
      s_count[j * 4 + w] = first_count;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int a = 0; a < kFlattenItems * 4; ++a) {
      const int root = s_root[a];
      if (root < 0) continue;
      int c = s_count[a];
      for (int b = a + 1; b < kFlattenItems * 4; ++b) {
        if (s_root[b] == root) {
          c += s_count[b];
          s_root[b] = -1;
        }
      }
      atomicAdd(counts + root, c);
    }
  }
}

// (count, label) as one key whose maximum is the larger count and, among equal counts, the smaller label
__device__ __forceinline__ unsigned long long cc_key(int count, int label) { return (unsigned long long)(unsigned)count << 32 | (unsigned)(0x7fffffff - label); }

// One lane per lattice point, after the counts are complete: the workgroup's inside points, roots, and best key
__global__ void __launch_bounds__(256) cc_partials_kernel(long long n, const int* __restrict__ labels, const int* __restrict__ counts, int* __restrict__ part_inside,
                                                          int* __restrict__ part_roots, unsigned long long* __restrict__ part_best) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int l = i < n ? labels[i] : -1;
  const bool root = l >= 0 && l == (int)i;
  int n_in, n_roots;
  block_scan_256(l >= 0 ? 1 : 0, &n_in);
  block_scan_256(root ? 1 : 0, &n_roots);
  unsigned long long best = root ? cc_key(counts[i], l) : 0ull;
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long u = __shfl_down(best, o);
    best = u > best ? u : best;
  }
  __shared__ unsigned long long wave_best[4];
  if ((threadIdx.x & 63) == 0) wave_best[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k) best = wave_best[k] > best ? wave_best[k] : best;
    part_inside[blockIdx.x] = n_in;
    part_roots[blockIdx.x] = n_roots;
    part_best[blockIdx.x] = best;
  }
}

// One workgroup: stats = inside points, components, label of the largest (-1 without an inside point), its point count
__global__ void __launch_bounds__(1024) cc_stats_kernel(long long nblk, const int* __restrict__ part_inside, const int* __restrict__ part_roots,
                                                        const unsigned long long* __restrict__ part_best, long long* __restrict__ stats_ws, long long* __restrict__ stats_dev) {
  long long n_in = 0, n_roots = 0;
  unsigned long long best = 0;
  for (long long j = threadIdx.x; j < nblk; j += 1024) {
    n_in += part_inside[j];
    n_roots += part_roots[j];
    best = part_best[j] > best ? part_best[j] : best;
  }
  for (int o = 32; o > 0; o >>= 1) {
    n_in += __shfl_down(n_in, o);
    n_roots += __shfl_down(n_roots, o);
    const unsigned long long u = __shfl_down(best, o);
    best = u > best ? u : best;
  }
  __shared__ long long s_in[16], s_roots[16];
  __shared__ unsigned long long s_best[16];
  if ((threadIdx.x & 63) == 0) {
    s_in[threadIdx.x >> 6] = n_in;
    s_roots[threadIdx.x >> 6] = n_roots;
    s_best[threadIdx.x >> 6] = best;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 16; ++k) {
      n_in += s_in[k];
      n_roots += s_roots[k];
      best = s_best[k] > best ? s_best[k] : best;
    }
    const long long count = (long long)(best >> 32);
    const long long label = count > 0 ? 0x7fffffffll - (long long)(best & 0xffffffffull) : -1;
    const long long st[4] = {n_in, n_roots, label, count};
    for (int k = 0; k < 4; ++k) {
      stats_ws[k] = st[k];
      stats_dev[k] = st[k];
    }
  }
}

// One lane per lattice point: its value, or -inf for an inside point of a dropped component.  Bits are copied as bits; out may be vol.
__global__ void __launch_bounds__(256) cc_keep_kernel(const unsigned* vol_bits, const int* __restrict__ labels, const int* __restrict__ counts,
                                                      const long long* __restrict__ stats, long long n, int largest_only, int min_points, unsigned* out_bits) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  unsigned v = vol_bits[i];
  const int l = labels[i];
  if (l >= 0 && l < n) {
    const bool keep = largest_only ? (long long)l == stats[2] : counts[l] >= min_points;
    if (!keep) v = 0xff800000u;      // -inf
  }
  out_bits[i] = v;
}

// workspace: stats int64 [4] | counts int32 [n] | inside per workgroup int32 | roots per workgroup int32 | best key per workgroup uint64
struct CcWs {
  long long n, nblk;
  size_t stats, counts, part_inside, part_roots, part_best, bytes;
};
CcWs cc_ws(int n0, int n1, int n2) {
  CcWs w;
  w.n = (long long)n0 * n1 * n2;
  w.nblk = (w.n + 255) / 256;
  size_t off = 0;
  w.stats = off; off += 256;
  w.counts = off; off += up256((size_t)w.n * sizeof(int));
  w.part_inside = off; off += up256((size_t)w.nblk * sizeof(int));
  w.part_roots = off; off += up256((size_t)w.nblk * sizeof(int));
  w.part_best = off; off += up256((size_t)w.nblk * sizeof(unsigned long long));
  w.bytes = off;
  return w;
}

// ---- vertex clustering ---------------------------------------------------------------------------------------------------------------

struct ClusterFrame {
  float origin[3], spacing[3];
  int m[3];      // cluster cells per axis: ceil((n_j - 1) / factor)
  float factor;
};

// One lane per vertex: its cluster id, and its lattice coordinates (2^-16 units, int64) into the cluster's sums
__global__ void __launch_bounds__(256) cluster_vertices_kernel(const float* __restrict__ vertices, long long V, const ClusterFrame fr, int* __restrict__ cid,
                                                               unsigned long long* __restrict__ sums, int* __restrict__ members) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  int cell[3];
  long long q[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float u = __fsub_rn(vertices[v * 3 + j], fr.origin[j]) / fr.spacing[j];
    const float f = floorf(u / fr.factor);
    cell[j] = f >= (float)(fr.m[j] - 1) ? fr.m[j] - 1 : (f > 0.0f ? (int)f : 0);      // a NaN falls into cell 0
    const double qd = (double)u * 65536.0;
    q[j] = fabs(qd) < 0x1p62 ? llrint(qd) : 0ll;                                       // a non-finite or absurd coordinate adds 0
  }
  const int c = (cell[0] * fr.m[1] + cell[1]) * fr.m[2] + cell[2];
  cid[v] = c;
#pragma unroll
  for (int j = 0; j < 3; ++j) atomicAdd(sums + (long long)c * 3 + j, (unsigned long long)q[j]);      // two's complement: signed sums
  atomicAdd(members + c, 1);
}

// 1: the face survives (three different clusters); 0: it collapses; -1: an index outside [0, V)
__device__ __forceinline__ int face_state(const int* __restrict__ faces, long long f, long long V, const int* __restrict__ cid, int c[3]) {
  int ok = 1;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int x = faces[f * 3 + j];
    if (x < 0 || x >= V) ok = 0;
    else c[j] = cid[x];
  }
  if (!ok) return -1;
  return c[0] != c[1] && c[1] != c[2] && c[0] != c[2] ? 1 : 0;
}

// One lane per face: marks the clusters of a surviving face as referenced; the workgroup's count of surviving faces; faces with an index
// out of range are counted into *bad and referenced nowhere
__global__ void __launch_bounds__(256) cluster_faces_count_kernel(const int* __restrict__ faces, long long F, long long V, const int* __restrict__ cid,
                                                                  int* __restrict__ used, int* __restrict__ block_counts, long long* __restrict__ bad) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  int c[3] = {0, 0, 0};
  const int st = f < F ? face_state(faces, f, V, cid, c) : 0;
  if (st == 1) {
#pragma unroll
    for (int j = 0; j < 3; ++j) used[c[j]] = 1;      // every writer stores the same 1
  }
  const unsigned long long bad_lanes = __ballot(st < 0);
  if (bad_lanes && (threadIdx.x & 63) == __ffsll((long long)bad_lanes) - 1) atomicAdd((unsigned long long*)bad, (unsigned long long)__popcll(bad_lanes));
  int total;
  block_scan_256(st == 1 ? 1 : 0, &total);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

// One lane per cluster: the workgroup's count of referenced clusters
__global__ void __launch_bounds__(256) cluster_used_count_kernel(const int* __restrict__ used, long long ncl, int* __restrict__ block_counts) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  int total;
  block_scan_256(c < ncl ? used[c] : 0, &total);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

// One lane per cluster: the new vertex number of a referenced cluster (ascending cluster id), -1 for the others
__global__ void __launch_bounds__(256) cluster_number_kernel(const int* __restrict__ used, const int* __restrict__ block_prefix, long long ncl, int* __restrict__ newid) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  const int u = c < ncl ? used[c] : 0;
  int total;
  const int before = block_scan_256(u, &total);
  if (c < ncl) newid[c] = u ? block_prefix[blockIdx.x] + before : -1;
}

// One lane per cluster: the mean of a referenced cluster's members, back in the mesh's coordinates
__global__ void __launch_bounds__(256) cluster_emit_vertices_kernel(const long long* __restrict__ sums, const int* __restrict__ members, const int* __restrict__ newid,
                                                                    long long ncl, const ClusterFrame fr, long long n_vertices, float* __restrict__ vertices) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= ncl) return;
  const long long slot = newid[c];
  if (slot < 0 || slot >= n_vertices) return;
  const double denom = (double)members[c] * 65536.0;      // a referenced cluster has a member
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double mean = (double)sums[c * 3 + j] / denom;
    vertices[slot * 3 + j] = (float)((double)fr.origin[j] + mean * (double)fr.spacing[j]);
  }
}

// One lane per face: a surviving face, re-indexed, at the slot its workgroup's prefix and the scan within the workgroup give
__global__ void __launch_bounds__(256) cluster_emit_faces_kernel(const int* __restrict__ faces, long long F, long long V, const int* __restrict__ cid,
                                                                 const int* __restrict__ newid, const int* __restrict__ block_prefix, long long n_faces,
                                                                 int* __restrict__ faces_out) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  int c[3] = {0, 0, 0};
  const int keep = f < F && face_state(faces, f, V, cid, c) == 1 ? 1 : 0;
  int total;
  const long long slot = (long long)block_prefix[blockIdx.x] + block_scan_256(keep, &total);
  if (!keep || slot >= n_faces) return;
#pragma unroll
  for (int j = 0; j < 3; ++j) faces_out[slot * 3 + j] = newid[c[j]];
}

// workspace: totals int64 [3] (vertices, faces, faces with an index out of range) | sums int64 [ncl][3] | members int32 [ncl] | used int32 [ncl] |
//            newid int32 [ncl] | cid int32 [V] | cluster block counts int32 | face block counts int32
struct ClusterWs {
  long long ncl, nblk_c, nblk_f;
  int m[3];
  size_t totals, sums, members, used, newid, cid, blocks_c, blocks_f, bytes;
};
ClusterWs cluster_ws(long long V, long long F, int n0, int n1, int n2, int factor) {
  ClusterWs w;
  const int n[3] = {n0, n1, n2};
  for (int j = 0; j < 3; ++j) w.m[j] = (n[j] - 1 + factor - 1) / factor;
  w.ncl = (long long)w.m[0] * w.m[1] * w.m[2];
  w.nblk_c = (w.ncl + 255) / 256;
  w.nblk_f = (F + 255) / 256;
  size_t off = 0;
  w.totals = off; off += 256;
  w.sums = off; off += up256((size_t)w.ncl * 3 * sizeof(long long));
  w.members = off; off += up256((size_t)w.ncl * sizeof(int));
  w.used = off; off += up256((size_t)w.ncl * sizeof(int));
  w.newid = off; off += up256((size_t)w.ncl * sizeof(int));
  w.cid = off; off += up256((size_t)V * sizeof(int));
  w.blocks_c = off; off += up256((size_t)w.nblk_c * sizeof(int));
  w.blocks_f = off; off += up256((size_t)w.nblk_f * sizeof(int));
  w.bytes = off;
  return w;
}

ClusterFrame cluster_frame(const ClusterWs& w, const float* origin, const float* spacing, int factor) {
  ClusterFrame fr;
  for (int j = 0; j < 3; ++j) {
    fr.origin[j] = origin[j];
    fr.spacing[j] = spacing[j];
    fr.m[j] = w.m[j];
  }
  fr.factor = (float)factor;
  return fr;
}

}  // namespace

size_t components_workspace_bytes(int n0, int n1, int n2) { return cc_ws(n0, n1, n2).bytes; }

int launch_volume_components(const float* vol, int n0, int n1, int n2, float iso, void* workspace, int* labels, long long* stats_dev, void* stream) {
  const CcWs w = cc_ws(n0, n1, n2);
  char* ws = (char*)workspace;
  const Lattice L = {n0, n1, n2, w.n};
  int* counts = (int*)(ws + w.counts);
  int* part_inside = (int*)(ws + w.part_inside);
  int* part_roots = (int*)(ws + w.part_roots);
  unsigned long long* part_best = (unsigned long long*)(ws + w.part_best);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)w.nblk), block(256);
  hipLaunchKernelGGL(cc_init_kernel, grid, block, 0, s, vol, w.n, iso, labels, counts);
  hipLaunchKernelGGL(cc_join_kernel, grid, block, 0, s, vol, L, iso, labels);
  hipLaunchKernelGGL(cc_flatten_count_kernel, dim3((unsigned)((w.n + 256 * kFlattenItems - 1) / (256 * kFlattenItems))), block, 0, s, w.n, labels, counts);
  hipLaunchKernelGGL(cc_partials_kernel, grid, block, 0, s, w.n, (const int*)labels, (const int*)counts, part_inside, part_roots, part_best);
  hipLaunchKernelGGL(cc_stats_kernel, dim3(1), dim3(1024), 0, s, w.nblk, (const int*)part_inside, (const int*)part_roots, (const unsigned long long*)part_best,
                     (long long*)(ws + w.stats), stats_dev);
  return check_launch("volume components launch");
}

int launch_volume_keep_components(const float* vol, const int* labels, const void* workspace, int n0, int n1, int n2, int largest_only, int min_points,
                                  float* vol_out, void* stream) {
  const CcWs w = cc_ws(n0, n1, n2);
  const char* ws = (const char*)workspace;
  hipLaunchKernelGGL(cc_keep_kernel, dim3((unsigned)w.nblk), dim3(256), 0, (hipStream_t)stream, (const unsigned*)vol, labels, (const int*)(ws + w.counts),
                     (const long long*)(ws + w.stats), w.n, largest_only, min_points, (unsigned*)vol_out);
  return check_launch("volume keep components launch");
}

size_t cluster_workspace_bytes(long long V, long long F, int n0, int n1, int n2, int factor) { return cluster_ws(V, F, n0, n1, n2, factor).bytes; }

// [dev] vertices, faces, faces with an index out of range: what launch_mesh_cluster_count left in the workspace
const long long* cluster_workspace_totals(const void* workspace) { return (const long long*)workspace; }

int launch_mesh_cluster_count(const float* vertices, long long V, const int* faces, long long F, const float* origin, const float* spacing, int n0, int n1,
                              int n2, int factor, void* workspace, long long* counts_dev, void* stream) {
  const ClusterWs w = cluster_ws(V, F, n0, n1, n2, factor);
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  long long* totals = (long long*)(ws + w.totals);
  if (hipError_t e = hipMemsetAsync(totals, 0, 256, s)) return hip_fail(e, "mesh cluster workspace clear");
  if (F == 0) {      // no face references a vertex: an empty result, nothing to launch
    if (hipError_t e = hipMemsetAsync(counts_dev, 0, 3 * sizeof(long long), s)) return hip_fail(e, "mesh cluster counts clear");
    return FENERF_OK;
  }
  // sums, members and used are adjacent: one clear
  if (hipError_t e = hipMemsetAsync(ws + w.sums, 0, w.newid - w.sums, s)) return hip_fail(e, "mesh cluster workspace clear");
  const ClusterFrame fr = cluster_frame(w, origin, spacing, factor);
  int* cid = (int*)(ws + w.cid);
  int* used = (int*)(ws + w.used);
  int* blocks_c = (int*)(ws + w.blocks_c);
  int* blocks_f = (int*)(ws + w.blocks_f);
  if (V > 0)
    hipLaunchKernelGGL(cluster_vertices_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, s, vertices, V, fr, cid, (unsigned long long*)(ws + w.sums),
                       (int*)(ws + w.members));
  hipLaunchKernelGGL(cluster_faces_count_kernel, dim3((unsigned)w.nblk_f), dim3(256), 0, s, faces, F, V, (const int*)cid, used, blocks_f, totals + 2);
  hipLaunchKernelGGL(cluster_used_count_kernel, dim3((unsigned)w.nblk_c), dim3(256), 0, s, (const int*)used, w.ncl, blocks_c);
  hipLaunchKernelGGL(block_counts_scan_kernel, dim3(2), dim3(1024), 0, s, blocks_c, w.nblk_c, blocks_f, w.nblk_f, totals, counts_dev);
  hipLaunchKernelGGL(cluster_number_kernel, dim3((unsigned)w.nblk_c), dim3(256), 0, s, (const int*)used, (const int*)blocks_c, w.ncl, (int*)(ws + w.newid));
  if (int rc = check_launch("mesh cluster count launch")) return rc;
  if (hipError_t e = hipMemcpyAsync(counts_dev + 2, totals + 2, sizeof(long long), hipMemcpyDeviceToDevice, s)) return hip_fail(e, "mesh cluster counts copy");
  return FENERF_OK;
}

int launch_mesh_cluster_emit(const int* faces, long long V, long long F, const float* origin, const float* spacing, int n0, int n1, int n2, int factor,
                             const void* workspace, long long n_vertices, long long n_faces, float* vertices_out, int* faces_out, void* stream) {
  const ClusterWs w = cluster_ws(V, F, n0, n1, n2, factor);
  const char* ws = (const char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const int* newid = (const int*)(ws + w.newid);
  if (n_vertices > 0) {
    const ClusterFrame fr = cluster_frame(w, origin, spacing, factor);
    hipLaunchKernelGGL(cluster_emit_vertices_kernel, dim3((unsigned)w.nblk_c), dim3(256), 0, s, (const long long*)(ws + w.sums), (const int*)(ws + w.members), newid,
                       w.ncl, fr, n_vertices, vertices_out);
  }
  if (n_faces > 0)
    hipLaunchKernelGGL(cluster_emit_faces_kernel, dim3((unsigned)w.nblk_f), dim3(256), 0, s, faces, F, V, (const int*)(ws + w.cid), newid,
                       (const int*)(ws + w.blocks_f), n_faces, faces_out);
  return check_launch("mesh cluster emit launch");
}

}  // namespace fenerf
