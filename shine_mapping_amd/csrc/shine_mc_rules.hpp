// shine_mc_rules.hpp — the per-cube rules of DESIGN.md "Meshing" that the dense marching cubes (shine_mc.hip) and the
// sparse-brick one (shine_mc_sparse.hip) share: which corner a crossing edge collapses onto, which triangles of a case are
// degenerate, and the 256-lane block scan both use to place their outputs.  Include it INSIDE the translation unit's
// anonymous namespace, after shine_mc_tables.hpp.
#pragma once

// Edge e of a cube with corner values c: the corner (0-7) its vertex collapses onto, or -1 for a vertex of its own.  (Only
// called for crossing edges.)
__device__ __forceinline__ int edge_collapse(const float c[8], float level, int e) {
  const int c0 = MC_EDGE_BASE[e], c1 = c0 | (1 << (e >> 2));
  if (c[c0] > level) return c[c1] == level ? c1 : -1;
  return c[c0] == level ? c0 : -1;
}

__device__ __forceinline__ bool tri_degenerate(const float c[8], float level, int e0, int e1, int e2) {
  const int k0 = edge_collapse(c, level, e0), k1 = edge_collapse(c, level, e1), k2 = edge_collapse(c, level, e2);
  return (k0 >= 0 && (k0 == k1 || k0 == k2)) || (k1 >= 0 && k1 == k2);
}

__device__ __forceinline__ int cube_tri_count(const float c[8], float level, int cs) {
  int n = 0;
  const int nt = MC_NTRI[cs];
  for (int k = 0; k < nt; ++k)
    n += tri_degenerate(c, level, MC_TRI[cs][3 * k], MC_TRI[cs][3 * k + 1], MC_TRI[cs][3 * k + 2]) ? 0 : 1;
  return n;
}

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// exclusive prefix of `v` over the 256 lanes of the block; `total` = the block's sum
__device__ __forceinline__ int block_excl_scan(int v, int& total, int* lds4) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int inc = wave_incl_scan(v, lane);
  if (lane == 63) lds4[w] = inc;
  __syncthreads();
  int off = 0;
  for (int k = 0; k < w; ++k) off += lds4[k];
  total = lds4[0] + lds4[1] + lds4[2] + lds4[3];
  __syncthreads();
  return off + inc - v;
}
