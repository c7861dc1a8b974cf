// shine_mc.hip — marching cubes on a dense fp32 grid [X, Y, Z] (C order, z fastest): the isosurface half of the reference's
// Mesher.mc_mesh (utils/mesher.py:200-222, skimage.measure.marching_cubes(level, allow_degenerate=False, mask=)).
//
// Rules (DESIGN.md "Meshing"): a grid value is "in" iff v > level; cube (x, y, z) is processed iff it lies inside the grid and
// mask[x, y, z] is set (no mask: every cube).  One vertex per crossing edge used by a processed cube, at p0 + t * axis,
// t = (level - v0) / (v1 - v0) in fp32, index units; an edge whose OUT end sits exactly on the level collapses onto that
// point's "corner vertex", and a triangle that then repeats a vertex is not emitted.  Vertices are ordered by owner point
// (corner vertex, +x, +y, +z edge), faces by cube, then by table order (csrc/shine_mc_tables.hpp).  No atomic decides where an
// output goes: the same input gives the same bits.  The per-point and per-cube rules themselves are in shine_mc_rules.hpp, shared
// with shine_mc_sparse.hip; this file gives them a view of the global grid and says which cubes are processed.
//
// Three passes over tiles of MC_TILE = 1024 grid points (256 lanes x 4):
//   classify  one lane per point: the owned-vertex bits (4) and the cube's non-degenerate triangle count (<= 5) packed in a
//             byte; per-tile vertex / face sums; the totals for the host (count call); tiles in XCD-contiguous order
//   scan      the tile sums (prim_scan_int, shine_prims.hip)
//   emit      tiles with nothing to write return at once; active tiles rebuild their in-tile prefix from the packed bytes, write
//             the vertices and each point's first vertex id (verts pass), then the faces, whose ids come from those bases
//             (faces pass: it reads other tiles' bases, hence its own launch)
#include "shine_internal.hpp"
#include "shine_mc_tables.hpp"

namespace {

#include "shine_mc_rules.hpp"  // FieldView, classify_bits, cube_triangles, the block reductions

constexpr int MC_THREADS = 256;
constexpr int MC_TILE = 4 * MC_THREADS;

struct McGrid {
  const float* v;
  const unsigned char* mask;  // nullptr: every cube is processed
  long long X, Y, Z, N;
  float level;
};

// (x, y, z) of point tile_base + o, 0 <= o < MC_TILE: the tile's first point is split once per block (wave-uniform 64-bit
// divisions), each lane then carries its offset with 32-bit divisions (Y, Z < 2^30, checked by the host entry points)
__device__ __forceinline__ void point_xyz(const McGrid& g, long long tile_base, int o, long long& x, long long& y, long long& z) {
  const long long yz = g.Y * g.Z;
  const long long x0 = tile_base / yz;
  const long long r = tile_base - x0 * yz;
  const unsigned y0 = (unsigned)(r / g.Z), z0 = (unsigned)(r - (long long)y0 * g.Z);
  const unsigned zz = z0 + (unsigned)o;
  const unsigned q = zz / (unsigned)g.Z;
  const unsigned yy = y0 + q;
  const unsigned q2 = yy / (unsigned)g.Y;
  z = zz - q * (unsigned)g.Z;
  y = yy - q2 * (unsigned)g.Y;
  x = x0 + q2;
}

// cube (x + dx, y + dy, z + dz) of point i = (x, y, z), d in {-1, 0}
__device__ __forceinline__ bool cube_processed(const McGrid& g, long long i, long long x, long long y, long long z, int dx, int dy,
                                               int dz) {
  x += dx;
  y += dy;
  z += dz;
  if (x < 0 || y < 0 || z < 0 || x >= g.X - 1 || y >= g.Y - 1 || z >= g.Z - 1) return false;
  return !g.mask || g.mask[i + dx * g.Y * g.Z + dy * g.Z + dz] != 0;
}

__device__ __forceinline__ FieldView<long long> grid_view(const McGrid& g) { return {g.v, g.Y * g.Z, g.Z, g.level}; }

// the processed flags of the 8 cubes that contain point i = (x, y, z): bit (dx | dy << 1 | dz << 2) = cube (x-1+dx, y-1+dy, z-1+dz)
__device__ __forceinline__ unsigned cubes_processed(const McGrid& g, long long i, long long x, long long y, long long z) {
  unsigned proc = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    proc |= (cube_processed(g, i, x, y, z, (k & 1) - 1, ((k >> 1) & 1) - 1, ((k >> 2) & 1) - 1) ? 1u : 0u) << k;
  return proc;
}

// The classify launch has 8 * ceil(tiles / 8) blocks; blocks that share an XCD (the same blockIdx % 8) take one contiguous eighth
// of the tiles, so the neighbouring rows and planes a point reads stay in one XCD's L2 instead of being fetched into several.
// Measured neutral so far (the pass is bound by its chain of dependent loads, not by HBM traffic); kept for
// when that chain is shortened.  Placement only changes speed: each tile has exactly one block.
__global__ __launch_bounds__(MC_THREADS) void k_mc_classify(McGrid g, long long tiles, unsigned char* __restrict__ packed,
                                                            int* __restrict__ tile_v, int* __restrict__ tile_f,
                                                            unsigned long long* __restrict__ totals) {
  __shared__ int red[2][4];
  const long long per = (tiles + 7) / 8;
  const long long tile = (long long)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
  if (tile >= tiles) return;
  const long long base = tile * MC_TILE;
  const FieldView<long long> f = grid_view(g);
  int nv = 0, nf = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int o = k * MC_THREADS + threadIdx.x;  // lanes along z: coalesced loads
    const long long i = base + o;
    unsigned char b = 0;
    if (i < g.N) {
      long long x, y, z;
      point_xyz(g, base, o, x, y, z);
      b = classify_bits(f, i, cubes_processed(g, i, x, y, z));
    }
    packed[i] = b;  // (the tail of the last tile is written as zeros: the emit passes read whole tiles)
    nv += __popc(b & 15u);
    nf += b >> 4;
  }
  block_sum2(nv, nf, red);
  if (threadIdx.x == 0) {
    tile_v[tile] = nv;
    tile_f[tile] = nf;
    // integer totals for the host's size query (order-independent: no output position depends on them)
    if (nv) atomicAdd(totals, (unsigned long long)nv);
    if (nf) atomicAdd(totals + 1, (unsigned long long)nf);
  }
}

__global__ __launch_bounds__(MC_THREADS) void k_mc_emit_verts(McGrid g, const unsigned char* __restrict__ packed,
                                                              const int* __restrict__ tile_v, const int* __restrict__ tile_vbase,
                                                              int* __restrict__ vbase, float* __restrict__ verts) {
  __shared__ int lds4[4];
  if (tile_v[blockIdx.x] == 0) return;  // surfaces are sparse
  const long long i0 = (long long)blockIdx.x * MC_TILE + 4 * threadIdx.x;
  const unsigned w4 = *reinterpret_cast<const unsigned*>(packed + i0);
  const unsigned vmask = w4 & 0x0f0f0f0fu;
  int total;
  int id = tile_vbase[blockIdx.x] + block_excl_scan(__popc(vmask), total, lds4);
  if (!vmask) return;
  const long long sx = g.Y * g.Z, sy = g.Z;
  for (int k = 0; k < 4; ++k) {
    const unsigned bits = (w4 >> (8 * k)) & 15u;
    if (!bits) continue;
    const long long i = i0 + k;
    long long x, y, z;
    point_xyz(g, (long long)blockIdx.x * MC_TILE, 4 * threadIdx.x + k, x, y, z);
    vbase[i] = id;
    const float px = (float)x, py = (float)y, pz = (float)z;
    const float v0 = g.v[i];
    if (bits & 1u) {
      verts[3 * (long long)id] = px;
      verts[3 * (long long)id + 1] = py;
      verts[3 * (long long)id + 2] = pz;
      ++id;
    }
    const long long stride[3] = {sx, sy, 1};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!(bits & (2u << a))) continue;
      const float v1 = g.v[i + stride[a]];
      const float t = (g.level - v0) / (v1 - v0);
      verts[3 * (long long)id] = a == 0 ? px + t : px;
      verts[3 * (long long)id + 1] = a == 1 ? py + t : py;
      verts[3 * (long long)id + 2] = a == 2 ? pz + t : pz;
      ++id;
    }
  }
}

__global__ __launch_bounds__(MC_THREADS) void k_mc_emit_faces(McGrid g, const unsigned char* __restrict__ packed,
                                                              const int* __restrict__ tile_f, const int* __restrict__ tile_fbase,
                                                              const int* __restrict__ vbase, int* __restrict__ faces) {
  __shared__ int lds4[4];
  if (tile_f[blockIdx.x] == 0) return;
  const long long i0 = (long long)blockIdx.x * MC_TILE + 4 * threadIdx.x;
  const unsigned w4 = *reinterpret_cast<const unsigned*>(packed + i0);
  const unsigned fcnt = ((w4 >> 4) & 15u) + ((w4 >> 12) & 15u) + ((w4 >> 20) & 15u) + (w4 >> 28);
  int total;
  long long fid = tile_fbase[blockIdx.x] + block_excl_scan((int)fcnt, total, lds4);
  if (!fcnt) return;
  const FieldView<long long> f = grid_view(g);
  const VertexIds<long long> ids = {vbase, packed};
  for (int k = 0; k < 4; ++k) {
    if (!((w4 >> (8 * k + 4)) & 15u)) continue;
    cube_triangles(f, i0 + k, ids, [&](int, const int id[3]) {
#pragma unroll
      for (int j = 0; j < 3; ++j) faces[3 * fid + j] = id[j];
      ++fid;
    });
  }
}

struct McWork {
  unsigned char* packed;
  int* vbase;
  int *tile_v, *tile_f, *tile_vbase, *tile_fbase;
  unsigned long long* totals;
  void* scan_tmp;
  size_t scan_bytes;
  size_t bytes;
};

McWork mc_layout(void* base, long long N, hipStream_t st) {
  const size_t tiles = (size_t)((N + MC_TILE - 1) / MC_TILE);
  McWork w = {};
  shine::Arena a(base);
  w.packed = a.take<unsigned char>(tiles * MC_TILE);
  w.vbase = a.take<int>((size_t)N);
  w.tile_v = a.take<int>(tiles);
  w.tile_f = a.take<int>(tiles);
  w.tile_vbase = a.take<int>(tiles);
  w.tile_fbase = a.take<int>(tiles);
  w.totals = a.take<unsigned long long>(2);
  (void)shine::prim_scan_int(nullptr, w.scan_bytes, nullptr, nullptr, tiles, st);
  w.scan_tmp = a.take_bytes(w.scan_bytes);
  w.bytes = a.bytes();
  return w;
}

int mc_check(const float* sdf, int64_t nx, int64_t ny, int64_t nz, size_t* workspace_bytes, const char* what) {
  if (nx < 0 || ny < 0 || nz < 0) return shine::set_error(SHINE_E_INVALID, what);
  if (nx > 0 && ny > 0 && nz > 0 && !sdf) return shine::set_error(SHINE_E_INVALID, what);
  if (nx && ny && nz && (nx > (1ll << 40) / ny / nz)) return shine::set_error(SHINE_E_INVALID, what);
  if (ny >= (1ll << 30) || nz >= (1ll << 30)) return shine::set_error(SHINE_E_INVALID, what);
  (void)workspace_bytes;
  return SHINE_OK;
}

}  // namespace

extern "C" int shine_mc_count(const float* sdf, const uint8_t* mask, int64_t nx, int64_t ny, int64_t nz, float level,
                              void* workspace, size_t* workspace_bytes, int64_t* counts_out, void* stream) {
  if (!workspace_bytes) return shine::set_error(SHINE_E_INVALID, "shine_mc_count: null workspace_bytes");
  if (mc_check(sdf, nx, ny, nz, workspace_bytes, "shine_mc_count: bad grid (negative size, null sdf, > 2^40 points or ny / nz >= 2^30)"))
    return SHINE_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const long long N = nx * ny * nz;
  McWork w = mc_layout(workspace, N, st);
  if (workspace && !counts_out) return shine::set_error(SHINE_E_INVALID, "shine_mc_count: null counts_out");
  SHINE_WORKSPACE_GATE(w.bytes, workspace, workspace_bytes, "shine_mc_count");
  counts_out[0] = counts_out[1] = 0;
  if (N == 0) return SHINE_OK;
  const long long tiles = (N + MC_TILE - 1) / MC_TILE;
  McGrid g = {sdf, mask, nx, ny, nz, N, level};
  SHINE_HIP_CHECK(hipMemsetAsync(w.totals, 0, 16, st));
  hipLaunchKernelGGL(k_mc_classify, dim3((unsigned)(8 * ((tiles + 7) / 8))), dim3(MC_THREADS), 0, st, g, (long long)tiles, w.packed,
                     w.tile_v, w.tile_f, w.totals);
  SHINE_HIP_CHECK(hipGetLastError());
  return scan_and_read_totals(w.tile_v, w.tile_vbase, w.tile_f, w.tile_fbase, (size_t)tiles, w.scan_tmp, w.scan_bytes, w.totals, counts_out,
                              "shine_mc_count: the mesh has 2^31 or more vertices or faces (int32 ids)", st);
}

extern "C" int shine_mc_emit(const float* sdf, const uint8_t* mask, int64_t nx, int64_t ny, int64_t nz, float level,
                             void* workspace, size_t workspace_bytes, float* verts_out, int32_t* faces_out, void* stream) {
  if (mc_check(sdf, nx, ny, nz, &workspace_bytes, "shine_mc_emit: bad grid (negative size, null sdf, > 2^40 points or ny / nz >= 2^30)"))
    return SHINE_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const long long N = nx * ny * nz;
  if (N == 0) return SHINE_OK;
  McWork w = mc_layout(workspace, N, st);
  SHINE_WORKSPACE_FITS(w.bytes, workspace, workspace_bytes, "shine_mc_emit");
  if (!verts_out || !faces_out) return shine::set_error(SHINE_E_INVALID, "shine_mc_emit: null output");
  const long long tiles = (N + MC_TILE - 1) / MC_TILE;
  McGrid g = {sdf, mask, nx, ny, nz, N, level};
  hipLaunchKernelGGL(k_mc_emit_verts, dim3((unsigned)tiles), dim3(MC_THREADS), 0, st, g, w.packed, w.tile_v, w.tile_vbase, w.vbase,
                     verts_out);
  SHINE_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_mc_emit_faces, dim3((unsigned)tiles), dim3(MC_THREADS), 0, st, g, w.packed, w.tile_f, w.tile_fbase, w.vbase,
                     faces_out);
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}
