// shine_mc_rules.hpp — the rules of DESIGN.md "Meshing", once, for the dense marching cubes (shine_mc.hip) and the sparse-brick
// one (shine_mc_sparse.hip): a cube's corner values and case, which corner a crossing edge collapses onto, which triangles of a
// case are degenerate, a point's classify byte, the walk over a cube's triangles with their vertex ids, and the block
// reductions / the totals read-back both use.  Include it INSIDE the translation unit's anonymous namespace, after
// shine_internal.hpp and shine_mc_tables.hpp.
//
// The rules read the field through a VIEW, which is all that differs between the two: the dense kernels read the global fp32 grid
// with 64-bit indices, FieldView<long long>{g.v, Y * Z, Z, level}; the brick kernels read the staged brick and its apron in LDS
// with 32-bit ones, FieldView<int>{sv, B1 * B1, B1, level}.  Which cubes are processed is the caller's business (the grid's
// mask, or the brick's own cubes only): the rules take the answer as bits.
#pragma once

template <class I>
struct FieldView {
  typedef I index;
  const float* v;
  I sx, sy;  // index steps along x and y (z: 1)
  float level;
  __device__ __forceinline__ float at(I i) const { return v[i]; }
  __device__ __forceinline__ I step(int axis) const { return axis == 0 ? sx : axis == 1 ? sy : (I)1; }
  // corner k of the cube at i: i + (k & 1, k >> 1 & 1, k >> 2 & 1)
  __device__ __forceinline__ I corner(I i, int k) const { return i + (k & 1) * sx + ((k >> 1) & 1) * sy + ((k >> 2) & 1); }
};

// The cube whose lowest corner is point i: its 8 corner values and case.
template <class V>
__device__ __forceinline__ int view_cube_case(const V& f, typename V::index i, float c[8]) {
  int cs = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    c[k] = f.at(f.corner(i, k));
    cs |= (c[k] > f.level ? 1 : 0) << k;
  }
  return cs;
}

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

// Point i = (x, y, z), given the processed flags of the 8 cubes that contain it — proc bit (dx | dy << 1 | dz << 2) = cube
// (x - 1 + dx, y - 1 + dy, z - 1 + dz) — returns bits 0-3 = those cubes use its corner vertex / +x / +y / +z edge vertex;
// bits 4-7 = non-degenerate triangles of cube (x, y, z).
template <class V>
__device__ __forceinline__ unsigned char classify_bits(const V& f, typename V::index i, unsigned proc) {
  if (!proc) return 0;
  const float v0 = f.at(i);
  const bool in0 = v0 > f.level;
  unsigned bits = 0;
  bool corner = false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    // the cubes around the axis-a edge FROM this point have d_a = 1, those around the edge INTO it d_a = 0.  A processed cube
    // lies inside the field with all its corners, so `up` / `down` being set is the only bounds check the far point needs.
    unsigned up = 0, down = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) ((k >> a) & 1 ? up : down) |= proc & (1u << k);
    if (up) {
      const float v1 = f.at(i + f.step(a));
      if (in0 != (v1 > f.level)) {
        if (in0 ? v1 != f.level : v0 != f.level) bits |= 2u << a;
        else if (!in0) corner = true;  // collapses onto this point
      }
    }
    if (down && v0 == f.level && f.at(i - f.step(a)) > f.level) corner = true;
  }
  bits |= corner ? 1u : 0u;
  if (proc & 0x80u) {  // cube (x, y, z) itself
    float c[8];
    const int cs = view_cube_case(f, i, c);
    if (cs != 0 && cs != 255) bits |= (unsigned)cube_tri_count(c, f.level, cs) << 4;
  }
  return (unsigned char)bits;
}

// The non-degenerate triangles of the cube at point i, in table order: emit(table position, the three vertex ids).  `ids` knows
// the classify pass's results: ids.first(q) = the id of point q's first vertex, ids.bits(q) = its classify byte.  A point's
// vertices are numbered corner vertex, +x, +y, +z edge, the owned ones only.
template <class V, class Ids, class Emit>
__device__ __forceinline__ void cube_triangles(const V& f, typename V::index i, const Ids& ids, Emit emit) {
  float c[8];
  const int cs = view_cube_case(f, i, c);
  const int nt = MC_NTRI[cs];
  for (int t = 0; t < nt; ++t) {
    const int e[3] = {MC_TRI[cs][3 * t], MC_TRI[cs][3 * t + 1], MC_TRI[cs][3 * t + 2]};
    if (tri_degenerate(c, f.level, e[0], e[1], e[2])) continue;
    int id[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int col = edge_collapse(c, f.level, e[j]);
      if (col >= 0) {
        id[j] = ids.first(f.corner(i, col));  // (the corner vertex comes first)
      } else {
        const typename V::index q = f.corner(i, MC_EDGE_BASE[e[j]]);
        const int a = e[j] >> 2;
        id[j] = ids.first(q) + __popc((ids.bits(q) & 15u) & ((2u << a) - 1u));
      }
    }
    emit(t, id);
  }
}

// first = each point's first vertex id, bits = each point's classify byte, indexed like the view
template <class I>
struct VertexIds {
  const int* first_id;
  const unsigned char* packed;
  __device__ __forceinline__ int first(I q) const { return first_id[q]; }
  __device__ __forceinline__ unsigned bits(I q) const { return packed[q]; }
};

// the sums of nv and of nf over the 256 lanes of the block, valid in thread 0
__device__ __forceinline__ void block_sum2(int& nv, int& nf, int (*red)[4]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) {
    nv += __shfl_xor(nv, o, 64);
    nf += __shfl_xor(nf, o, 64);
  }
  if (lane == 0) {
    red[0][w] = nv;
    red[1][w] = nf;
  }
  __syncthreads();
  nv = red[0][0] + red[0][1] + red[0][2] + red[0][3];
  nf = red[1][0] + red[1][1] + red[1][2] + red[1][3];
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

// The end of a count call (host): the per-block vertex / face sums scanned into bases, the two totals read back into
// counts_out; refuses a mesh whose ids do not fit int32 with the caller's message.
int scan_and_read_totals(const int* sum_v, int* base_v, const int* sum_f, int* base_f, size_t n, void* scan_tmp, size_t scan_bytes,
                         const unsigned long long* totals, int64_t* counts_out, const char* too_large, hipStream_t st) {
  size_t sb = scan_bytes;
  SHINE_HIP_CHECK(shine::prim_scan_int(scan_tmp, sb, sum_v, base_v, n, st));
  sb = scan_bytes;
  SHINE_HIP_CHECK(shine::prim_scan_int(scan_tmp, sb, sum_f, base_f, n, st));
  unsigned long long tot[2] = {0, 0};
  SHINE_HIP_CHECK(hipMemcpyAsync(tot, totals, 16, hipMemcpyDeviceToHost, st));
  SHINE_HIP_CHECK(hipStreamSynchronize(st));
  counts_out[0] = (int64_t)tot[0];
  counts_out[1] = (int64_t)tot[1];
  if (tot[0] >= (1ull << 31) || tot[1] >= (1ull << 31)) return shine::set_error(SHINE_E_INVALID, too_large);
  return SHINE_OK;
}
