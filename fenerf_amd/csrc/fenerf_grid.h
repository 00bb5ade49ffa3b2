// The trilinear corner walk of the 3-D feature grid: sample_from_3dgrid (siren.py:314-330) = grid_sample, trilinear, zeros padding,
// align_corners=True.  The gather's transposes (the float-atomic, the fused and the deterministic scatters), the non-finite pass and
// the coordinate gradient all take a point's eight corners from here, so they agree on which corners exist and on their weights bit
// for bit (FP contraction is off for the whole library).  The two forward gathers (siren_kernel, siren16w_kernel) write the same
// statements out in place -- through these functions the compiler places their tile prologue differently -- and must match this file.
// What a kernel does per corner -- blend channels, atomic add, int64 add, the +-1 factors of the coordinate gradient -- stays at its
// call site, inside its own unrolled loop:
//
//   const GridCell k = grid_cell(qx, qy, qz, gd, gh, gw);
//   for (int c = 0; c < 8; ++c) {
//     const GridCorner n = grid_corner(k, c);
//     if (n.ok) { ... grid_voxel(k, n) ... n.wx * n.wy * n.wz ... }
//   }
#pragma once
#include <hip/hip_runtime.h>

namespace fenerf {

// a point in grid coordinates: q in [-1, 1] (UniformBoxWarp applied) maps to [0, size - 1] per axis
struct GridCell {
  int gd, gh, gw;
  float ix, iy, iz;   // continuous voxel coordinates
  float x0, y0, z0;   // their floors: the lower corner
};
__device__ __forceinline__ GridCell grid_cell(float qx, float qy, float qz, int gd, int gh, int gw) {
  GridCell k;
  k.gd = gd; k.gh = gh; k.gw = gw;
  k.ix = ((qx + 1.f) / 2.f) * (float)(gw - 1);
  k.iy = ((qy + 1.f) / 2.f) * (float)(gh - 1);
  k.iz = ((qz + 1.f) / 2.f) * (float)(gd - 1);
  k.x0 = floorf(k.ix); k.y0 = floorf(k.iy); k.z0 = floorf(k.iz);
  return k;
}

// corner c = 4 cz + 2 cy + cx of the cell (cx = 1: the upper neighbour along x)
struct GridCorner {
  int cx, cy, cz;
  float xi, yi, zi;   // integer-valued voxel coordinates
  float wx, wy, wz;   // per-axis weights; the corner's weight is wx * wy * wz
  bool ok;            // inside the grid.  Six ordered comparisons: every one is false for a NaN coordinate, which so selects no corner;
                      // an upper neighbour that leaves the grid from a point exactly on the last plane has weight 0 and is skipped too
};
__device__ __forceinline__ GridCorner grid_corner(const GridCell& k, int c) {
  GridCorner n;
  n.cz = c >> 2; n.cy = (c >> 1) & 1; n.cx = c & 1;
  n.xi = k.x0 + n.cx; n.yi = k.y0 + n.cy; n.zi = k.z0 + n.cz;
  n.wx = n.cx ? (k.ix - k.x0) : (k.x0 + 1.f - k.ix);
  n.wy = n.cy ? (k.iy - k.y0) : (k.y0 + 1.f - k.iy);
  n.wz = n.cz ? (k.iz - k.z0) : (k.z0 + 1.f - k.iz);
  n.ok = n.xi >= 0.f && n.xi <= (float)(k.gw - 1) && n.yi >= 0.f && n.yi <= (float)(k.gh - 1) && n.zi >= 0.f && n.zi <= (float)(k.gd - 1);
  return n;
}
// voxel index of an in-range corner in a [D][H][W][...] grid (only meaningful when n.ok: the casts of an out-of-range float are not)
__device__ __forceinline__ long long grid_voxel(const GridCell& k, const GridCorner& n) {
  return ((long long)(int)n.zi * k.gh + (int)n.yi) * k.gw + (int)n.xi;
}

}  // namespace fenerf
