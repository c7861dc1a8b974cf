// shine_mesh.hip — mesh post-processing on the device, after marching cubes (shine_mc.hip):
//   vertex normals   open3d's TriangleMesh.compute_vertex_normals (utils/mesher.py:283, :353): per vertex the sum of its faces'
//                    (v1 - v0) x (v2 - v0), in face order, normalised.  A gather, not a scatter: the (vertex, face) pairs are
//                    sorted (prim_sort_keys_u64) and each vertex sums its own run, so the result is the same bits every run
//                    and works on any mesh (also after vertices were removed and the ids compacted).
//   cluster filter   Mesher.filter_isolated_vertices (utils/mesher.py:240-251): open3d's cluster_connected_triangles joins
//                    triangles that share an undirected edge; the triangles of clusters with fewer than min_tri triangles are
//                    removed (remove_triangles_by_mask: the order of the rest kept, vertices kept).  Edge keys (min v, max v)
//                    sorted with their triangle ids (prim_sort_pairs_u64); triangles with equal keys are united by hooking the
//                    larger root onto the smaller (atomicMin) and pointer jumping until nothing changes, so every cluster's
//                    root is its smallest triangle; cluster ids are the roots' ranks (open3d numbers clusters in that order).
#include "shine_internal.hpp"

namespace {

constexpr int T = 256;

unsigned grid_of(long long n) { return (unsigned)((n + T - 1) / T); }

unsigned bits_for(long long n) {  // bits that hold 0..n-1
  unsigned b = 1;
  while (b < 63 && (1ll << b) < n) ++b;
  return b;
}

// ---------------------------------------------------------------- normals
__global__ void k_face_normals(const double* __restrict__ v, const int* __restrict__ f, long long nf, double* __restrict__ fn,
                               unsigned long long* __restrict__ keys) {
  const long long t = (long long)blockIdx.x * T + threadIdx.x;
  if (t >= nf) return;
  const int a = f[3 * t], b = f[3 * t + 1], c = f[3 * t + 2];
  const double e1x = v[3ll * b] - v[3ll * a], e1y = v[3ll * b + 1] - v[3ll * a + 1], e1z = v[3ll * b + 2] - v[3ll * a + 2];
  const double e2x = v[3ll * c] - v[3ll * a], e2y = v[3ll * c + 1] - v[3ll * a + 1], e2z = v[3ll * c + 2] - v[3ll * a + 2];
  fn[3 * t] = e1y * e2z - e1z * e2y;
  fn[3 * t + 1] = e1z * e2x - e1x * e2z;
  fn[3 * t + 2] = e1x * e2y - e1y * e2x;
  keys[3 * t] = ((unsigned long long)(unsigned)a << 32) | (unsigned long long)t;
  keys[3 * t + 1] = ((unsigned long long)(unsigned)b << 32) | (unsigned long long)t;
  keys[3 * t + 2] = ((unsigned long long)(unsigned)c << 32) | (unsigned long long)t;
}

// runs of equal vertex in the sorted keys: [start[v], end[v])
__global__ void k_runs(const unsigned long long* __restrict__ keys, long long n, long long* __restrict__ start,
                       long long* __restrict__ end) {
  const long long j = (long long)blockIdx.x * T + threadIdx.x;
  if (j >= n) return;
  const unsigned long long v = keys[j] >> 32;
  if (j == 0 || (keys[j - 1] >> 32) != v) start[v] = j;
  if (j == n - 1 || (keys[j + 1] >> 32) != v) end[v] = j + 1;
}

__global__ void k_vertex_normals(const unsigned long long* __restrict__ keys, const long long* __restrict__ start,
                                 const long long* __restrict__ end, const double* __restrict__ fn, long long nv,
                                 double* __restrict__ out) {
  const long long v = (long long)blockIdx.x * T + threadIdx.x;
  if (v >= nv) return;
  double x = 0.0, y = 0.0, z = 0.0;
  for (long long j = start[v]; j < end[v]; ++j) {
    const long long t = (long long)(keys[j] & 0xffffffffull);
    x += fn[3 * t];
    y += fn[3 * t + 1];
    z += fn[3 * t + 2];
  }
  const double sq = x * x + y * y + z * z;
  if (sq > 0.0) {  // (Eigen's normalize(): a zero vector stays zero)
    const double n = sqrt(sq);
    x /= n;
    y /= n;
    z /= n;
  }
  out[3 * v] = x;
  out[3 * v + 1] = y;
  out[3 * v + 2] = z;
}

// ---------------------------------------------------------------- clusters
__global__ void k_edge_keys(const int* __restrict__ f, long long nf, unsigned long long* __restrict__ keys,
                            unsigned long long* __restrict__ vals) {
  const long long t = (long long)blockIdx.x * T + threadIdx.x;
  if (t >= nf) return;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const unsigned a = (unsigned)f[3 * t + j], b = (unsigned)f[3 * t + (j + 1) % 3];
    const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
    keys[3 * t + j] = ((unsigned long long)lo << 32) | hi;
    vals[3 * t + j] = (unsigned long long)t;
  }
}

__global__ void k_iota(int* __restrict__ p, long long n) {
  const long long t = (long long)blockIdx.x * T + threadIdx.x;
  if (t < n) p[t] = (int)t;
}

__device__ __forceinline__ int find_root(const int* parent, int x) {
  int p = parent[x];
  while (p != x) {
    x = p;
    p = parent[x];
  }
  return x;
}

__global__ void k_hook(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ vals, long long n,
                       int* parent, int* __restrict__ changed) {
  const long long j = (long long)blockIdx.x * T + threadIdx.x;
  if (j == 0 || j >= n || keys[j] != keys[j - 1]) return;
  const int ra = find_root(parent, (int)vals[j - 1]), rb = find_root(parent, (int)vals[j]);
  if (ra == rb) return;
  atomicMin(parent + (ra > rb ? ra : rb), ra < rb ? ra : rb);  // parents only decrease: no cycle, roots end as minima
  *changed = 1;
}

__global__ void k_jump(int* parent, long long n) {
  const long long t = (long long)blockIdx.x * T + threadIdx.x;
  if (t < n) parent[t] = find_root(parent, (int)t);
}

__global__ void k_root_flags(const int* __restrict__ parent, long long n, unsigned char* __restrict__ flags) {
  const long long t = (long long)blockIdx.x * T + threadIdx.x;
  if (t < n) flags[t] = parent[t] == (int)t ? 1 : 0;
}

__global__ void k_cluster_count(const int* __restrict__ parent, const int* __restrict__ rank, long long n,
                                int* __restrict__ cluster, int* __restrict__ counts) {
  const long long t = (long long)blockIdx.x * T + threadIdx.x;
  if (t >= n) return;
  const int c = rank[parent[t]];
  cluster[t] = c;
  // one atomic per distinct cluster in the wave: most triangles belong to one big cluster, and lane-by-lane adds on its counter
  // serialise (an integer count: the same whatever the order)
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(1);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int lc = __shfl(c, leader, 64);
    const unsigned long long same = __ballot(c == lc) & todo;
    if (lane == leader) atomicAdd(counts + lc, (int)__popcll(same));
    todo &= ~same;
  }
}

__global__ void k_keep_flags(const int* __restrict__ cluster, const int* __restrict__ counts, long long n, int min_tri,
                             unsigned char* __restrict__ keep) {
  const long long t = (long long)blockIdx.x * T + threadIdx.x;
  if (t < n) keep[t] = counts[cluster[t]] >= min_tri ? 1 : 0;
}

__global__ void k_compact(const int* __restrict__ f, const unsigned char* __restrict__ keep, const int* __restrict__ pos,
                          long long n, int* __restrict__ out) {
  const long long t = (long long)blockIdx.x * T + threadIdx.x;
  if (t >= n || !keep[t]) return;
  const long long o = pos[t];
  out[3 * o] = f[3 * t];
  out[3 * o + 1] = f[3 * t + 1];
  out[3 * o + 2] = f[3 * t + 2];
}

}  // namespace

extern "C" int shine_mesh_vertex_normals(const double* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                         void* workspace, size_t* workspace_bytes, double* normals_out, void* stream) {
  if (!workspace_bytes || n_verts < 0 || n_faces < 0 || n_verts >= (1ll << 31) || n_faces >= (1ll << 31))
    return shine::set_error(SHINE_E_INVALID, "shine_mesh_vertex_normals: bad sizes (V and F must be < 2^31)");
  hipStream_t st = (hipStream_t)stream;
  const long long nk = 3 * n_faces;
  shine::Arena c(workspace);
  auto* k0 = c.take<unsigned long long>(nk);
  auto* k1 = c.take<unsigned long long>(nk);
  auto* fn = c.take<double>(nk);
  auto* start = c.take<long long>(n_verts);
  auto* end = c.take<long long>(n_verts);
  size_t sort_bytes = 0;
  const unsigned end_bit = 32 + bits_for(n_verts);
  SHINE_HIP_CHECK(shine::prim_sort_keys_u64(nullptr, sort_bytes, nullptr, nullptr, (size_t)nk, 0u, end_bit, st));
  void* tmp = c.take_bytes(sort_bytes);
  SHINE_WORKSPACE_GATE(c.bytes(), workspace, workspace_bytes, "shine_mesh_vertex_normals");
  if (n_verts == 0) return SHINE_OK;
  if (!verts || !normals_out || (n_faces && !faces)) return shine::set_error(SHINE_E_INVALID, "shine_mesh_vertex_normals: null argument");
  SHINE_HIP_CHECK(hipMemsetAsync(start, 0, n_verts * 8, st));
  SHINE_HIP_CHECK(hipMemsetAsync(end, 0, n_verts * 8, st));
  if (n_faces) {
    hipLaunchKernelGGL(k_face_normals, dim3(grid_of(n_faces)), dim3(T), 0, st, verts, faces, (long long)n_faces, fn, k0);
    SHINE_HIP_CHECK(hipGetLastError());
    SHINE_HIP_CHECK(shine::prim_sort_keys_u64(tmp, sort_bytes, k0, k1, (size_t)nk, 0u, end_bit, st));
    hipLaunchKernelGGL(k_runs, dim3(grid_of(nk)), dim3(T), 0, st, k1, nk, start, end);
    SHINE_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_vertex_normals, dim3(grid_of(n_verts)), dim3(T), 0, st, k1, start, end, fn, (long long)n_verts, normals_out);
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}

extern "C" int shine_mesh_cluster_filter(const int32_t* faces, int64_t n_faces, int32_t min_tri, void* workspace,
                                         size_t* workspace_bytes, int32_t* cluster_out, int32_t* faces_out, int64_t* kept_out,
                                         void* stream) {
  if (!workspace_bytes || n_faces < 0 || n_faces >= (1ll << 31))
    return shine::set_error(SHINE_E_INVALID, "shine_mesh_cluster_filter: bad size (F must be < 2^31)");
  hipStream_t st = (hipStream_t)stream;
  const long long nk = 3 * n_faces;
  shine::Arena c(workspace);
  auto* k0 = c.take<unsigned long long>(nk);
  auto* k1 = c.take<unsigned long long>(nk);
  auto* v0 = c.take<unsigned long long>(nk);
  auto* v1 = c.take<unsigned long long>(nk);
  int* parent = c.take<int>(n_faces);
  int* rank = c.take<int>(n_faces);
  int* cluster = c.take<int>(n_faces);
  int* counts = c.take<int>(n_faces);
  int* pos = c.take<int>(n_faces);
  auto* flags = c.take<unsigned char>(n_faces);
  int* changed = c.take<int>(1);
  size_t sort_bytes = 0, scan_bytes = 0;
  SHINE_HIP_CHECK(shine::prim_sort_pairs_u64(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, (size_t)nk, 0u, 64u, st));
  SHINE_HIP_CHECK(shine::prim_scan_flags(nullptr, scan_bytes, nullptr, nullptr, (size_t)n_faces, st));
  const size_t tmp_bytes = sort_bytes > scan_bytes ? sort_bytes : scan_bytes;
  void* tmp = c.take_bytes(tmp_bytes);
  SHINE_WORKSPACE_GATE(c.bytes(), workspace, workspace_bytes, "shine_mesh_cluster_filter");
  if (!kept_out) return shine::set_error(SHINE_E_INVALID, "shine_mesh_cluster_filter: null kept_out");
  *kept_out = 0;
  if (n_faces == 0) return SHINE_OK;
  if (!faces || !faces_out) return shine::set_error(SHINE_E_INVALID, "shine_mesh_cluster_filter: null argument");
  const long long nf = n_faces;
  hipLaunchKernelGGL(k_edge_keys, dim3(grid_of(nf)), dim3(T), 0, st, faces, nf, k0, v0);
  SHINE_HIP_CHECK(hipGetLastError());
  size_t sb = tmp_bytes;
  SHINE_HIP_CHECK(shine::prim_sort_pairs_u64(tmp, sb, k0, k1, v0, v1, (size_t)nk, 0u, 64u, st));
  hipLaunchKernelGGL(k_iota, dim3(grid_of(nf)), dim3(T), 0, st, parent, nf);
  SHINE_HIP_CHECK(hipGetLastError());
  // every round hooks at least one root lower while two united triangles still have different roots; the rounds a mesh needs
  // grow like log(cluster diameter), the cap only guards against a broken invariant
  int done = 0;
  for (int round = 0; round < 4096 && !done; ++round) {
    SHINE_HIP_CHECK(hipMemsetAsync(changed, 0, 4, st));
    hipLaunchKernelGGL(k_hook, dim3(grid_of(nk)), dim3(T), 0, st, k1, v1, nk, parent, changed);
    SHINE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_jump, dim3(grid_of(nf)), dim3(T), 0, st, parent, nf);
    SHINE_HIP_CHECK(hipGetLastError());
    int h = 0;
    SHINE_HIP_CHECK(hipMemcpyAsync(&h, changed, 4, hipMemcpyDeviceToHost, st));
    SHINE_HIP_CHECK(hipStreamSynchronize(st));
    done = h == 0;
  }
  if (!done) return shine::set_error(SHINE_E_STATE, "shine_mesh_cluster_filter: union-find did not converge");
  hipLaunchKernelGGL(k_root_flags, dim3(grid_of(nf)), dim3(T), 0, st, parent, nf, flags);
  SHINE_HIP_CHECK(hipGetLastError());
  sb = tmp_bytes;
  SHINE_HIP_CHECK(shine::prim_scan_flags(tmp, sb, flags, rank, (size_t)nf, st));
  SHINE_HIP_CHECK(hipMemsetAsync(counts, 0, nf * 4, st));
  int* cl = cluster_out ? cluster_out : cluster;
  hipLaunchKernelGGL(k_cluster_count, dim3(grid_of(nf)), dim3(T), 0, st, parent, rank, nf, cl, counts);
  SHINE_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_keep_flags, dim3(grid_of(nf)), dim3(T), 0, st, cl, counts, nf, (int)min_tri, flags);
  SHINE_HIP_CHECK(hipGetLastError());
  sb = tmp_bytes;
  SHINE_HIP_CHECK(shine::prim_scan_flags(tmp, sb, flags, pos, (size_t)nf, st));
  hipLaunchKernelGGL(k_compact, dim3(grid_of(nf)), dim3(T), 0, st, faces, flags, pos, nf, faces_out);
  SHINE_HIP_CHECK(hipGetLastError());
  int last[2] = {0, 0};
  unsigned char lastf = 0;
  SHINE_HIP_CHECK(hipMemcpyAsync(&last[0], pos + nf - 1, 4, hipMemcpyDeviceToHost, st));
  SHINE_HIP_CHECK(hipMemcpyAsync(&lastf, flags + nf - 1, 1, hipMemcpyDeviceToHost, st));
  SHINE_HIP_CHECK(hipStreamSynchronize(st));
  *kept_out = (int64_t)last[0] + lastf;
  return SHINE_OK;
}
