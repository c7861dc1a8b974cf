// shine_mc_sparse.hip — marching cubes over a BRICK SET: n bricks of B^3 fp32 values (+ an optional B^3 mask) at B-aligned
// origins inside a virtual grid [X, Y, Z] that is never allocated.  A grid point no brick covers has value 0 and mask 0 — the
// zero fill of the dense grid Mesher.octree_grid_device assembles — and the result is, bit for bit, what shine_mc.hip gives on
// that dense grid: the same rules (DESIGN.md "Meshing"; shine_mc_rules.hpp, instantiated over a view of LDS), tables and order.
// Memory is proportional to the bricks and to the surface, not to X * Y * Z.
//
// Every cube belongs to the brick that holds its lowest corner, so only that brick's mask decides whether it is processed; the
// cubes on a brick's +x / +y / +z faces read values of up to 7 neighbour bricks (or zeros).  One workgroup per brick stages
// the (B + 1)^3 values of the brick and its apron in LDS, and everything after that reads LDS:
//   classify  (count call) one byte per apron point: which of its corner / +x / +y / +z vertices the brick's OWN processed
//             cubes use (4 bits) and, for a point that is a processed cube, its non-degenerate triangle count; per-brick sums,
//             a scan over the bricks, the totals for the host.  A brick whose apron does not change sign stops after staging.
//   emit      bricks with nothing to write return at once.  The others write one record per vertex they use,
//             (key = owner point's linear index * 4 + slot, value = record id << 32 | bits of t), and one per triangle,
//             (key = cube's linear index * 8 + table position, three record ids).  A vertex on a brick face is written by
//             every brick that uses it, with the same t (both compute it from the same two values).
//   order     prim_sort_pairs_u64 over the vertex keys, heads of equal-key runs flagged and scanned: a run's rank is the
//             vertex id, its key the position; each record learns its rank.  A second sort over the face keys puts the
//             triangles in dense order, their record ids replaced by ranks.  No atomic decides a position.
// The brick table (origins -> neighbour indices) is built on the host from the HOST origins array: a sort and seven merges.
#include <algorithm>
#include <utility>
#include <vector>

#include "shine_internal.hpp"

namespace {

#include "shine_mc_tables.hpp"  // (inside the namespace: shine_mc.hip owns the external copies of the tables)
#include "shine_mc_rules.hpp"

constexpr int SP_THREADS = 256;
constexpr int SP_MAX_B = 32;
constexpr int SP_CAP_SMALL = 16 * 16 * 16;  // apron floats of B <= 15: 16 KB of LDS, several workgroups per CU
constexpr int SP_CAP_LARGE = 33 * 33 * 33;  // B <= 32: 140 KB, one workgroup per CU

typedef unsigned long long u64;

struct SpGrid {
  const float* v;             // [n, B, B, B]
  const unsigned char* mask;  // [n, B, B, B] or nullptr: every cube of a brick is processed
  const long long* org;       // [n, 3] device copy of the origins
  const int* nbr;             // [n, 8]: brick at origin + B * (k & 1, k >> 1 & 1, k >> 2 & 1), -1 if none; [0] = itself
  long long X, Y, Z;
  int B, B1;  // B1 = B + 1: the apron's edge
  float level;
};

// the brick's values and its +x / +y / +z apron -> sv[(lx * B1 + ly) * B1 + lz]
__device__ __forceinline__ void stage_brick(const SpGrid& g, long long b, float* sv) {
  const int B = g.B, B1 = g.B1, n1 = B1 * B1 * B1;
  const long long B3 = (long long)B * B * B;
  for (int a = threadIdx.x; a < n1; a += SP_THREADS) {
    const int lz = a % B1, r = a / B1, ly = r % B1, lx = r / B1;
    const int which = (lx == B ? 1 : 0) | (ly == B ? 2 : 0) | (lz == B ? 4 : 0);
    const long long nb = which ? (long long)g.nbr[b * 8 + which] : b;
    float val = 0.f;
    if (nb >= 0) val = g.v[nb * B3 + ((lx == B ? 0 : lx) * B + (ly == B ? 0 : ly)) * B + (lz == B ? 0 : lz)];
    sv[a] = val;
  }
  __syncthreads();
}

// cube (cx, cy, cz) in brick coordinates: one of this brick's cubes, inside the grid, mask set
__device__ __forceinline__ bool sp_processed(const SpGrid& g, long long b, long long ox, long long oy, long long oz, int cx, int cy,
                                             int cz) {
  const int B = g.B;
  if ((unsigned)cx >= (unsigned)B || (unsigned)cy >= (unsigned)B || (unsigned)cz >= (unsigned)B) return false;
  if (ox + cx >= g.X - 1 || oy + cy >= g.Y - 1 || oz + cz >= g.Z - 1) return false;
  return !g.mask || g.mask[b * ((long long)B * B * B) + (cx * B + cy) * B + cz] != 0;
}

__device__ __forceinline__ FieldView<int> brick_view(const SpGrid& g, const float* sv) { return {sv, g.B1 * g.B1, g.B1, g.level}; }

// the processed flags of the 8 cubes that contain apron point a = (lx, ly, lz), the cubes of other bricks left out: bit
// (dx | dy << 1 | dz << 2) = cube (lx-1+dx, ly-1+dy, lz-1+dz).  (A processed cube of this brick has all its corners in the apron.)
__device__ __forceinline__ unsigned sp_cubes_processed(const SpGrid& g, long long b, long long ox, long long oy, long long oz, int a) {
  const int B1 = g.B1;
  const int lz = a % B1, r = a / B1, ly = r % B1, lx = r / B1;
  unsigned proc = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    proc |= (sp_processed(g, b, ox, oy, oz, lx - 1 + (k & 1), ly - 1 + ((k >> 1) & 1), lz - 1 + ((k >> 2) & 1)) ? 1u : 0u) << k;
  return proc;
}

template <int CAP>
__global__ __launch_bounds__(SP_THREADS) void k_sp_classify(SpGrid g, unsigned char* __restrict__ packed, int* __restrict__ brick_v,
                                                            int* __restrict__ brick_f, u64* __restrict__ totals) {
  __shared__ float sv[CAP];
  __shared__ int red[2][4];
  const long long b = blockIdx.x;
  const int n1 = g.B1 * g.B1 * g.B1;
  stage_brick(g, b, sv);
  int any_in = 0, any_out = 0;
  for (int a = threadIdx.x; a < n1; a += SP_THREADS) {
    const bool in = sv[a] > g.level;
    any_in |= in ? 1 : 0;
    any_out |= in ? 0 : 1;
  }
  const int has_in = __syncthreads_or(any_in), has_out = __syncthreads_or(any_out);
  if (!has_in || !has_out) {  // no edge crosses: nothing to write, and the emit pass never reads this brick's bytes
    if (threadIdx.x == 0) brick_v[b] = brick_f[b] = 0;
    return;
  }
  const long long ox = g.org[3 * b], oy = g.org[3 * b + 1], oz = g.org[3 * b + 2];
  const FieldView<int> f = brick_view(g, sv);
  int nv = 0, nf = 0;
  for (int a = threadIdx.x; a < n1; a += SP_THREADS) {
    const unsigned char c = classify_bits(f, a, sp_cubes_processed(g, b, ox, oy, oz, a));
    packed[b * n1 + a] = c;
    nv += __popc(c & 15u);
    nf += c >> 4;
  }
  block_sum2(nv, nf, red);
  if (threadIdx.x == 0) {
    brick_v[b] = nv;
    brick_f[b] = nf;
    // integer totals for the host's size query (order-independent: no output position depends on them)
    if (nv) atomicAdd(totals, (u64)nv);
    if (nf) atomicAdd(totals + 1, (u64)nf);
  }
}

struct SpRecords {
  u64 *vkeys, *vvals;  // [C] vertex records
  u64 *fkeys, *fvals;  // [F] face records: key, own index
  int* frec;           // [F, 3] vertex record ids of the triangle
};

template <int CAP>
__global__ __launch_bounds__(SP_THREADS) void k_sp_emit(SpGrid g, const unsigned char* __restrict__ packed,
                                                        const int* __restrict__ brick_v, const int* __restrict__ brick_f,
                                                        const int* __restrict__ brick_vbase, const int* __restrict__ brick_fbase,
                                                        int* vbase, SpRecords o) {
  __shared__ float sv[CAP];
  __shared__ int lds4[4];
  const long long b = blockIdx.x;
  if (brick_v[b] == 0 && brick_f[b] == 0) return;  // surfaces are sparse
  const int B1 = g.B1, n1 = B1 * B1 * B1;
  const int stride[3] = {B1 * B1, B1, 1};
  stage_brick(g, b, sv);
  const long long ox = g.org[3 * b], oy = g.org[3 * b + 1], oz = g.org[3 * b + 2];
  const unsigned char* pk = packed + b * n1;
  int* vb = vbase + b * n1;
  // vertex records, and every apron point's first record id
  int run = brick_vbase[b];
  for (int a0 = 0; a0 < n1; a0 += SP_THREADS) {
    const int a = a0 + threadIdx.x;
    const unsigned bits = a < n1 ? pk[a] & 15u : 0u;
    int total;
    int id = run + block_excl_scan(__popc(bits), total, lds4);
    run += total;
    if (!bits) continue;
    vb[a] = id;
    const int lz = a % B1, r = a / B1, ly = r % B1, lx = r / B1;
    const u64 lin = (u64)(((ox + lx) * g.Y + (oy + ly)) * g.Z + (oz + lz));
    const float v0 = sv[a];
    if (bits & 1u) {
      o.vkeys[id] = lin * 4;
      o.vvals[id] = (u64)id << 32;
      ++id;
    }
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      if (!(bits & (2u << ax))) continue;
      const float v1 = sv[a + stride[ax]];
      const float t = (g.level - v0) / (v1 - v0);
      o.vkeys[id] = lin * 4 + 1 + ax;
      o.vvals[id] = ((u64)id << 32) | (u64)__float_as_uint(t);
      ++id;
    }
  }
  if (brick_f[b] == 0) return;
  __syncthreads();  // the record ids above are read back by other lanes
  const FieldView<int> f = brick_view(g, sv);
  const VertexIds<int> ids = {vb, pk};
  long long frun = brick_fbase[b];
  for (int a0 = 0; a0 < n1; a0 += SP_THREADS) {
    const int a = a0 + threadIdx.x;
    const int cnt = a < n1 ? pk[a] >> 4 : 0;
    int total;
    long long fid = frun + block_excl_scan(cnt, total, lds4);
    frun += total;
    if (!cnt) continue;
    const int lz = a % B1, r = a / B1, ly = r % B1, lx = r / B1;
    const u64 lin = (u64)(((ox + lx) * g.Y + (oy + ly)) * g.Z + (oz + lz));
    cube_triangles(f, a, ids, [&](int t, const int id[3]) {
#pragma unroll
      for (int j = 0; j < 3; ++j) o.frec[3 * fid + j] = id[j];
      o.fkeys[fid] = lin * 8 + (u64)t;
      o.fvals[fid] = (u64)fid;
      ++fid;
    });
  }
}

__global__ __launch_bounds__(SP_THREADS) void k_sp_heads(const u64* __restrict__ keys, unsigned char* __restrict__ head, long long n) {
  const long long i = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
  if (i < n) head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

// sorted record i: rank = heads in front of it (+ its own) - 1 = the vertex id; the run's head writes the position
__global__ __launch_bounds__(SP_THREADS) void k_sp_write_verts(const u64* __restrict__ keys, const u64* __restrict__ vals,
                                                               const unsigned char* __restrict__ head, const int* __restrict__ excl,
                                                               long long n, long long Y, long long Z, int* __restrict__ rank,
                                                               float* __restrict__ verts, long long* __restrict__ n_verts) {
  const long long i = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
  if (i >= n) return;
  const int h = head[i];
  const long long r = (long long)excl[i] + h - 1;
  rank[vals[i] >> 32] = (int)r;
  if (i == n - 1) *n_verts = r + 1;
  if (!h) return;
  const u64 key = keys[i];
  const int slot = (int)(key & 3u);
  const long long lin = (long long)(key >> 2);
  const long long yz = Y * Z;
  const long long x = lin / yz, rem = lin - x * yz;
  const long long y = rem / Z, z = rem - y * Z;
  const float t = __uint_as_float((unsigned)(vals[i] & 0xffffffffu));
  const float px = (float)x, py = (float)y, pz = (float)z;
  verts[3 * r] = slot == 1 ? px + t : px;
  verts[3 * r + 1] = slot == 2 ? py + t : py;
  verts[3 * r + 2] = slot == 3 ? pz + t : pz;
}

__global__ __launch_bounds__(SP_THREADS) void k_sp_write_faces(const u64* __restrict__ order, const int* __restrict__ frec,
                                                               const int* __restrict__ rank, long long n, long long n_records,
                                                               int* __restrict__ faces) {
  const long long j = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
  if (j >= n) return;
  const long long rec = (long long)order[j];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const unsigned id = (unsigned)frec[3 * rec + k];
    faces[3 * j + k] = id < (unsigned long long)n_records ? rank[id] : -1;  // (never out of the table, whatever the workspace held)
  }
}

struct SpWork {  // the count call's workspace: proportional to the bricks
  long long* org;
  int* nbr;
  unsigned char* packed;
  int* vbase;
  int *brick_v, *brick_f, *brick_vbase, *brick_fbase;
  u64* totals;
  void* scan_tmp;
  size_t scan_bytes;
  size_t bytes;
};

SpWork sp_layout(void* base, long long n_bricks, int B, hipStream_t st) {
  const size_t n = (size_t)n_bricks, n1 = (size_t)(B + 1) * (B + 1) * (B + 1);
  SpWork w = {};
  shine::Arena a(base);
  w.org = a.take<long long>(n * 3);
  w.nbr = a.take<int>(n * 8);
  w.packed = a.take<unsigned char>(n * n1);
  w.vbase = a.take<int>(n * n1);
  w.brick_v = a.take<int>(n);
  w.brick_f = a.take<int>(n);
  w.brick_vbase = a.take<int>(n);
  w.brick_fbase = a.take<int>(n);
  w.totals = a.take<u64>(2);
  (void)shine::prim_scan_int(nullptr, w.scan_bytes, nullptr, nullptr, n, st);
  w.scan_tmp = a.take_bytes(w.scan_bytes);
  w.bytes = a.bytes();
  return w;
}

struct SpScratch {  // the emit call's scratch: proportional to the surface
  u64 *vkeys, *vvals, *vkeys_s, *vvals_s;
  unsigned char* head;
  int *excl, *rank;
  u64 *fkeys, *fvals, *fkeys_s, *fvals_s;
  int* frec;
  long long* n_verts;
  void* tmp;
  size_t tmp_bytes;
  size_t bytes;
};

unsigned key_bits(u64 max_key) {
  unsigned b = 1;
  while (b < 64 && (max_key >> b)) ++b;
  return b;
}

SpScratch sp_scratch(void* base, long long n_records, long long n_faces, unsigned vbits, unsigned fbits, hipStream_t st) {
  const size_t C = (size_t)n_records, F = (size_t)n_faces;
  SpScratch s = {};
  shine::Arena a(base);
  s.vkeys = a.take<u64>(C);
  s.vvals = a.take<u64>(C);
  s.vkeys_s = a.take<u64>(C);
  s.vvals_s = a.take<u64>(C);
  s.head = a.take<unsigned char>(C);
  s.excl = a.take<int>(C);
  s.rank = a.take<int>(C);
  s.fkeys = a.take<u64>(F);
  s.fvals = a.take<u64>(F);
  s.fkeys_s = a.take<u64>(F);
  s.fvals_s = a.take<u64>(F);
  s.frec = a.take<int>(F * 3);
  s.n_verts = a.take<long long>(1);
  size_t sort_v = 0, sort_f = 0, scan = 0;
  (void)shine::prim_sort_pairs_u64(nullptr, sort_v, nullptr, nullptr, nullptr, nullptr, C, 0u, vbits, st);
  (void)shine::prim_sort_pairs_u64(nullptr, sort_f, nullptr, nullptr, nullptr, nullptr, F, 0u, fbits, st);
  (void)shine::prim_scan_flags(nullptr, scan, nullptr, nullptr, C, st);
  s.tmp_bytes = std::max(sort_v, std::max(sort_f, scan));
  s.tmp = a.take_bytes(s.tmp_bytes);
  s.bytes = a.bytes();
  return s;
}

// the arguments both calls share; everything here is host arithmetic
int sp_check(const float* values, int64_t n, int32_t B, int64_t nx, int64_t ny, int64_t nz, const char* what) {
  if (B < 1 || B > SP_MAX_B) return shine::set_error(SHINE_E_INVALID, what);
  if (n < 0 || n >= (1ll << 31) || nx < 0 || ny < 0 || nz < 0) return shine::set_error(SHINE_E_INVALID, what);
  if (n > 0 && !values) return shine::set_error(SHINE_E_INVALID, what);
  // face keys are cube index * 8 in 64 bits
  if (nx && ny && nz && ((unsigned __int128)nx * (unsigned __int128)ny * (unsigned __int128)nz >= ((unsigned __int128)1 << 60)))
    return shine::set_error(SHINE_E_INVALID, what);
  return SHINE_OK;
}

// origins (host) -> neighbour table; refuses origins that are negative, outside the grid, not multiples of B, or repeated
int sp_brick_table(const int64_t* org, int64_t n, int B, int64_t nx, int64_t ny, int64_t nz, std::vector<int>& nbr) {
  const long long nby = (ny + B - 1) / B, nbz = (nz + B - 1) / B;
  std::vector<std::pair<u64, int>> keys((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t x = org[3 * i], y = org[3 * i + 1], z = org[3 * i + 2];
    if (x < 0 || y < 0 || z < 0 || x >= nx || y >= ny || z >= nz)
      return shine::set_error(SHINE_E_INVALID, "shine_mc_sparse_count: a brick origin lies outside the grid");
    if (x % B || y % B || z % B)
      return shine::set_error(SHINE_E_INVALID, "shine_mc_sparse_count: a brick origin is not a multiple of the brick edge");
    keys[(size_t)i] = {(u64)((x / B * nby + y / B) * nbz + z / B), (int)i};
  }
  std::sort(keys.begin(), keys.end());
  for (size_t i = 1; i < keys.size(); ++i)
    if (keys[i].first == keys[i - 1].first)
      return shine::set_error(SHINE_E_INVALID, "shine_mc_sparse_count: two bricks have the same origin");
  nbr.assign((size_t)n * 8, -1);
  for (int64_t i = 0; i < n; ++i) nbr[(size_t)i * 8] = (int)i;
  // neighbour k of a brick has key + a constant: one merge over the sorted keys per direction
  for (int k = 1; k < 8; ++k) {
    const long long dx = k & 1, dy = (k >> 1) & 1, dz = (k >> 2) & 1;
    const u64 delta = (u64)((dx * nby + dy) * nbz + dz);
    size_t j = 0;
    for (size_t i = 0; i < keys.size(); ++i) {
      const int64_t* p = org + 3 * (int64_t)keys[i].second;
      if ((dy && p[1] / B + 1 >= nby) || (dz && p[2] / B + 1 >= nbz)) continue;  // (x needs no check: such a key is in no brick)
      const u64 want = keys[i].first + delta;
      while (j < keys.size() && keys[j].first < want) ++j;
      if (j < keys.size() && keys[j].first == want) nbr[(size_t)keys[i].second * 8 + k] = keys[j].second;
    }
  }
  return SHINE_OK;
}

template <int CAP>
void launch_classify(const SpGrid& g, long long n, const SpWork& w, hipStream_t st) {
  hipLaunchKernelGGL(k_sp_classify<CAP>, dim3((unsigned)n), dim3(SP_THREADS), 0, st, g, w.packed, w.brick_v, w.brick_f, w.totals);
}

template <int CAP>
void launch_emit(const SpGrid& g, long long n, const SpWork& w, const SpRecords& o, hipStream_t st) {
  hipLaunchKernelGGL(k_sp_emit<CAP>, dim3((unsigned)n), dim3(SP_THREADS), 0, st, g, w.packed, w.brick_v, w.brick_f, w.brick_vbase,
                     w.brick_fbase, w.vbase, o);
}

#define SP_BAD ": bad brick set (brick edge outside 1..32, negative count or extent, null values, or nx * ny * nz >= 2^60)"

}  // namespace

extern "C" int shine_mc_sparse_count(const float* values, const uint8_t* mask, const int64_t* origins, int64_t n, int32_t brick,
                                     int64_t nx, int64_t ny, int64_t nz, float level, void* workspace, size_t* workspace_bytes,
                                     int64_t* counts_out, void* stream) {
  if (!workspace_bytes) return shine::set_error(SHINE_E_INVALID, "shine_mc_sparse_count: null workspace_bytes");
  if (sp_check(values, n, brick, nx, ny, nz, "shine_mc_sparse_count" SP_BAD)) return SHINE_E_INVALID;
  if (n > 0 && !origins) return shine::set_error(SHINE_E_INVALID, "shine_mc_sparse_count: null origins");
  hipStream_t st = (hipStream_t)stream;
  try {
    std::vector<int> nbr;
    if (sp_brick_table(origins, n, brick, nx, ny, nz, nbr)) return SHINE_E_INVALID;
    SpWork w = sp_layout(workspace, n, brick, st);
    if (workspace && !counts_out) return shine::set_error(SHINE_E_INVALID, "shine_mc_sparse_count: null counts_out");
    SHINE_WORKSPACE_GATE(w.bytes, workspace, workspace_bytes, "shine_mc_sparse_count");
    counts_out[0] = counts_out[1] = 0;
    if (n == 0 || nx == 0 || ny == 0 || nz == 0) return SHINE_OK;
    hipError_t e = hipMemcpyAsync(w.org, origins, (size_t)n * 24, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(w.nbr, nbr.data(), (size_t)n * 32, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(w.totals, 0, 16, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // (the host arrays may go away after this call)
    SHINE_HIP_CHECK(e);
    SpGrid g = {values, mask, w.org, w.nbr, nx, ny, nz, brick, brick + 1, level};
    if ((brick + 1) * (brick + 1) * (brick + 1) <= SP_CAP_SMALL) launch_classify<SP_CAP_SMALL>(g, n, w, st);
    else launch_classify<SP_CAP_LARGE>(g, n, w, st);
    SHINE_HIP_CHECK(hipGetLastError());
    return scan_and_read_totals(w.brick_v, w.brick_vbase, w.brick_f, w.brick_fbase, (size_t)n, w.scan_tmp, w.scan_bytes, w.totals,
                                counts_out, "shine_mc_sparse_count: the mesh has 2^31 or more vertex records or faces (int32 ids)", st);
  } catch (const std::bad_alloc&) {
    return shine::set_error(SHINE_E_NOMEM, "shine_mc_sparse_count: out of host memory for the brick table");
  }
}

extern "C" int shine_mc_sparse_emit(const float* values, const uint8_t* mask, int64_t n, int32_t brick, int64_t nx, int64_t ny,
                                    int64_t nz, float level, void* workspace, size_t workspace_bytes, int64_t n_records,
                                    int64_t n_faces, void* scratch, size_t* scratch_bytes, float* verts_out, int32_t* faces_out,
                                    int64_t* n_verts_out, void* stream) {
  if (!scratch_bytes) return shine::set_error(SHINE_E_INVALID, "shine_mc_sparse_emit: null scratch_bytes");
  if (sp_check(values, n, brick, nx, ny, nz, "shine_mc_sparse_emit" SP_BAD)) return SHINE_E_INVALID;
  if (n_records < 0 || n_faces < 0 || n_records >= (1ll << 31) || n_faces >= (1ll << 31))
    return shine::set_error(SHINE_E_INVALID, "shine_mc_sparse_emit: record / face counts must be those of shine_mc_sparse_count");
  hipStream_t st = (hipStream_t)stream;
  const long long C = n_records, F = n_faces;
  const u64 points = (u64)nx * (u64)ny * (u64)nz;
  const unsigned vbits = key_bits(points * 4 - 1), fbits = key_bits(points * 8 - 1);
  SpScratch s = sp_scratch(scratch, C, F, vbits, fbits, st);
  if (!scratch) {  // (by hand, not SHINE_WORKSPACE_GATE: the scratch has its own message, after checks only a real call passes)
    *scratch_bytes = s.bytes;
    return SHINE_OK;
  }
  if (!n_verts_out) return shine::set_error(SHINE_E_INVALID, "shine_mc_sparse_emit: null n_verts_out");
  *n_verts_out = 0;
  if (n == 0 || (C == 0 && F == 0)) return SHINE_OK;
  if (C == 0) return shine::set_error(SHINE_E_INVALID, "shine_mc_sparse_emit: faces without vertex records");
  if (!verts_out || (F > 0 && !faces_out)) return shine::set_error(SHINE_E_INVALID, "shine_mc_sparse_emit: null output");
  if (*scratch_bytes < s.bytes) return shine::set_error(SHINE_E_INVALID, "shine_mc_sparse_emit: scratch too small");
  SpWork w = sp_layout(workspace, n, brick, st);
  SHINE_WORKSPACE_FITS(w.bytes, workspace, workspace_bytes, "shine_mc_sparse_emit");
  SpGrid g = {values, mask, w.org, w.nbr, nx, ny, nz, brick, brick + 1, level};
  SpRecords o = {s.vkeys, s.vvals, s.fkeys, s.fvals, s.frec};
  if ((brick + 1) * (brick + 1) * (brick + 1) <= SP_CAP_SMALL) launch_emit<SP_CAP_SMALL>(g, n, w, o, st);
  else launch_emit<SP_CAP_LARGE>(g, n, w, o, st);
  SHINE_HIP_CHECK(hipGetLastError());
  size_t tb = s.tmp_bytes;
  SHINE_HIP_CHECK(shine::prim_sort_pairs_u64(s.tmp, tb, s.vkeys, s.vkeys_s, s.vvals, s.vvals_s, (size_t)C, 0u, vbits, st));
  const unsigned cb = (unsigned)((C + SP_THREADS - 1) / SP_THREADS);
  hipLaunchKernelGGL(k_sp_heads, dim3(cb), dim3(SP_THREADS), 0, st, s.vkeys_s, s.head, C);
  SHINE_HIP_CHECK(hipGetLastError());
  tb = s.tmp_bytes;
  SHINE_HIP_CHECK(shine::prim_scan_flags(s.tmp, tb, s.head, s.excl, (size_t)C, st));
  hipLaunchKernelGGL(k_sp_write_verts, dim3(cb), dim3(SP_THREADS), 0, st, s.vkeys_s, s.vvals_s, s.head, s.excl, C, (long long)ny,
                     (long long)nz, s.rank, verts_out, s.n_verts);
  SHINE_HIP_CHECK(hipGetLastError());
  if (F > 0) {
    tb = s.tmp_bytes;
    SHINE_HIP_CHECK(shine::prim_sort_pairs_u64(s.tmp, tb, s.fkeys, s.fkeys_s, s.fvals, s.fvals_s, (size_t)F, 0u, fbits, st));
    hipLaunchKernelGGL(k_sp_write_faces, dim3((unsigned)((F + SP_THREADS - 1) / SP_THREADS)), dim3(SP_THREADS), 0, st, s.fvals_s,
                       s.frec, s.rank, F, C, faces_out);
    SHINE_HIP_CHECK(hipGetLastError());
  }
  long long nv = 0;
  SHINE_HIP_CHECK(hipMemcpyAsync(&nv, s.n_verts, 8, hipMemcpyDeviceToHost, st));
  SHINE_HIP_CHECK(hipStreamSynchronize(st));
  *n_verts_out = nv;
  return SHINE_OK;
}
