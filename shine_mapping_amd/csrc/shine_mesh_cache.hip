// shine_mesh_cache.hip — the device side of Mesher.update_octree_mesh's block cache: which feature rows changed
// since the last mesh, which query-level node blocks those rows (and new nodes) can have changed, and the write of freshly queried
// blocks into the cache.  Three memory-bound streaming kernels; every flag is a byte, every count an integer atomic.
//   rows diff     one launch over all featured levels, one lane per 32-byte feature row (two 16-byte loads, consecutive lanes on
//                 consecutive rows): flag = row is beyond the snapshot or differs from it BITWISE; the snapshot is rewritten only
//                 where the flag is set, so an unchanged map costs two reads of the tables and one byte per row.
//   mark dirty    launch 1, one lane per node of the query slot and of every finer slot: a node is dirty when it is new or one of
//                 its eight corner rows is flagged; a dirty node stores 1 at its query-level ancestor (key >> 3 per level, found
//                 by binary search in the sorted query keys; every writer stores the same byte).  Launch 2, one lane per query
//                 node: its ancestor in every coarser slot (binary search in that slot's sorted keys) is tested the same way;
//                 then the flags are counted (block count, one integer atomic per block).
//   scatter       one lane per grid point: block b of the queried chunk goes to block index[b] of the cache.
#include "shine_internal.hpp"

namespace {

constexpr int T = 256;

struct DiffArgs {
  const uint4* feat[SHINE_MAX_LEVELS];
  uint4* snap[SHINE_MAX_LEVELS];
  uint8_t* flag[SHINE_MAX_LEVELS];
  long long rows[SHINE_MAX_LEVELS];       // real rows of the table (without the trash row)
  long long snap_rows[SHINE_MAX_LEVELS];  // rows the snapshot holds
  unsigned int block0[SHINE_MAX_LEVELS + 1];  // first block of every level
  int n;
};

__device__ __forceinline__ bool differs(const uint4& a, const uint4& b) {
  return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) != 0u;
}

__global__ void __launch_bounds__(T) k_rows_diff(const DiffArgs a, unsigned long long* __restrict__ changed) {
  int s = 0;
  while (s + 1 < a.n && blockIdx.x >= a.block0[s + 1]) ++s;
  const long long i = (long long)(blockIdx.x - a.block0[s]) * T + threadIdx.x;
  int ch = 0;
  if (i < a.rows[s]) {
    const uint4 f0 = a.feat[s][2 * i], f1 = a.feat[s][2 * i + 1];
    if (i >= a.snap_rows[s]) {
      ch = 1;
    } else {
      const uint4 s0 = a.snap[s][2 * i], s1 = a.snap[s][2 * i + 1];
      ch = (differs(f0, s0) || differs(f1, s1)) ? 1 : 0;
    }
    if (ch) {
      a.snap[s][2 * i] = f0;
      a.snap[s][2 * i + 1] = f1;
    }
    a.flag[s][i] = (uint8_t)ch;
  }
  const int c = __syncthreads_count(ch);
  if (threadIdx.x == 0 && c) atomicAdd(&changed[s], (unsigned long long)c);
}

struct MarkArgs {
  const long long* keys[SHINE_MAX_LEVELS];    // node keys, insertion order
  const int* ids[SHINE_MAX_LEVELS];           // [n][8] corner rows
  const uint8_t* flags[SHINE_MAX_LEVELS];     // row flags of k_rows_diff
  const long long* sorted[SHINE_MAX_LEVELS];  // keys ascending (slots <= sq)
  const long long* perm[SHINE_MAX_LEVELS];    // sorted position -> insertion index
  long long n[SHINE_MAX_LEVELS], prev[SHINE_MAX_LEVELS], flag_rows[SHINE_MAX_LEVELS];
  unsigned int block0[SHINE_MAX_LEVELS + 1];  // launch 1: first block of slots sq .. n_levels - 1 (indexed by slot - sq)
  int n_levels, sq;
};

__device__ __forceinline__ bool row_changed(const MarkArgs& a, int s, int id) {
  // (an id outside the flags cannot come from a consistent table: treated as changed, never read)
  return (unsigned long long)(long long)id >= (unsigned long long)a.flag_rows[s] || a.flags[s][id] != 0;
}

__device__ __forceinline__ bool node_dirty(const MarkArgs& a, int s, long long j) {
  if (j >= a.prev[s]) return true;
  const int4* p = reinterpret_cast<const int4*>(a.ids[s] + 8 * j);
  const int4 lo = p[0], hi = p[1];
  return row_changed(a, s, lo.x) || row_changed(a, s, lo.y) || row_changed(a, s, lo.z) || row_changed(a, s, lo.w) ||
         row_changed(a, s, hi.x) || row_changed(a, s, hi.y) || row_changed(a, s, hi.z) || row_changed(a, s, hi.w);
}

// insertion index of `key` in slot s, or -1
__device__ __forceinline__ long long find_node(const MarkArgs& a, int s, long long key) {
  const long long* __restrict__ v = a.sorted[s];
  long long lo = 0, hi = a.n[s];
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (v[mid] < key) lo = mid + 1; else hi = mid;
  }
  if (lo >= a.n[s] || v[lo] != key) return -1;
  const long long j = a.perm[s][lo];
  return (j >= 0 && j < a.n[s]) ? j : -1;
}

__global__ void __launch_bounds__(T) k_mark_scatter(const MarkArgs a, uint8_t* __restrict__ dirty) {
  int r = 0;
  const int slots = a.n_levels - a.sq;
  while (r + 1 < slots && blockIdx.x >= a.block0[r + 1]) ++r;
  const int s = a.sq + r;
  const long long j = (long long)(blockIdx.x - a.block0[r]) * T + threadIdx.x;
  if (j >= a.n[s] || !node_dirty(a, s, j)) return;
  if (r == 0) {
    dirty[j] = 1;
    return;
  }
  const long long q = find_node(a, a.sq, a.keys[s][j] >> (3 * r));
  if (q >= 0) dirty[q] = 1;
}

__global__ void __launch_bounds__(T) k_mark_gather(const MarkArgs a, uint8_t* __restrict__ dirty,
                                                   unsigned long long* __restrict__ counts) {
  const long long q = (long long)blockIdx.x * T + threadIdx.x;
  int d = 0;
  if (q < a.n[a.sq]) {
    d = dirty[q] != 0;
    const long long key = a.keys[a.sq][q];
    for (int s = a.sq - 1; s >= 0 && !d; --s) {
      const long long j = find_node(a, s, key >> (3 * (a.sq - s)));
      if (j >= 0 && node_dirty(a, s, j)) d = 1;
    }
    if (d) dirty[q] = 1;
  }
  const int old = __syncthreads_count(d && q < a.prev[a.sq]);
  const int all = __syncthreads_count(d);
  if (threadIdx.x == 0) {
    if (old) atomicAdd(&counts[0], (unsigned long long)old);
    if (all) atomicAdd(&counts[1], (unsigned long long)all);
  }
}

__global__ void __launch_bounds__(T) k_blocks_scatter(const float* __restrict__ sdf, const uint8_t* __restrict__ mask,
                                                      const long long* __restrict__ index, long long total, long long k3,
                                                      long long capacity, float* __restrict__ values,
                                                      uint8_t* __restrict__ masks) {
  const long long i = (long long)blockIdx.x * T + threadIdx.x;
  if (i >= total) return;
  const long long b = i / k3, r = i - b * k3;
  const long long dst = index[b];
  if (dst < 0 || dst >= capacity) return;
  values[dst * k3 + r] = sdf[i];
  masks[dst * k3 + r] = mask ? (uint8_t)(mask[i] != 0) : (uint8_t)0;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

constexpr long long MAX_BLOCKS = (1ll << 31) - 1;

}  // namespace

extern "C" int shine_rows_diff(int32_t n_levels, const float* const* feats, float* const* snaps, const int64_t* rows,
                               const int64_t* snap_rows, uint8_t* const* flags, int64_t* changed, void* stream) {
  if (n_levels < 1 || n_levels > SHINE_MAX_LEVELS || !feats || !snaps || !rows || !snap_rows || !flags || !changed)
    return shine::set_error(SHINE_E_INVALID, "shine_rows_diff: 1..8 levels and non-null arrays");
  DiffArgs a{};
  a.n = n_levels;
  long long blocks = 0;
  for (int s = 0; s < n_levels; ++s) {
    const long long real = rows[s] - 1;  // the trash row, the last one, is never compared
    if (rows[s] < 1 || snap_rows[s] < 0)
      return shine::set_error(SHINE_E_INVALID, "shine_rows_diff: a table has at least its trash row; snapshot rows >= 0");
    if (real > 0 && (!feats[s] || !snaps[s] || !flags[s] || !aligned16(feats[s]) || !aligned16(snaps[s])))
      return shine::set_error(SHINE_E_INVALID, "shine_rows_diff: null or not 16-byte aligned table / snapshot / flags");
    a.feat[s] = reinterpret_cast<const uint4*>(feats[s]);
    a.snap[s] = reinterpret_cast<uint4*>(snaps[s]);
    a.flag[s] = flags[s];
    a.rows[s] = real;
    a.snap_rows[s] = snap_rows[s];
    a.block0[s] = (unsigned int)blocks;
    blocks += (real + T - 1) / T;
    if (blocks > MAX_BLOCKS) return shine::set_error(SHINE_E_INVALID, "shine_rows_diff: too many rows for one launch");
  }
  a.block0[n_levels] = (unsigned int)blocks;
  if (blocks == 0) return SHINE_OK;
  hipLaunchKernelGGL(k_rows_diff, dim3((unsigned int)blocks), dim3(T), 0, (hipStream_t)stream, a,
                     reinterpret_cast<unsigned long long*>(changed));
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}

extern "C" int shine_mesh_mark_dirty(int32_t n_levels, int32_t sq, const int64_t* const* node_keys, const int32_t* const* node_ids,
                                     const int64_t* n_nodes, const int64_t* prev_nodes, const uint8_t* const* row_flags,
                                     const int64_t* flag_rows, const int64_t* const* sorted_keys, const int64_t* const* sorted_perm,
                                     uint8_t* dirty_out, int64_t* counts_out, void* stream) {
  if (n_levels < 1 || n_levels > SHINE_MAX_LEVELS || sq < 0 || sq >= n_levels || !node_keys || !node_ids || !n_nodes ||
      !prev_nodes || !row_flags || !flag_rows || !sorted_keys || !sorted_perm || !counts_out)
    return shine::set_error(SHINE_E_INVALID, "shine_mesh_mark_dirty: 1..8 levels, 0 <= sq < levels, non-null arrays");
  MarkArgs a{};
  a.n_levels = n_levels;
  a.sq = sq;
  long long blocks = 0;
  for (int s = 0; s < n_levels; ++s) {
    if (n_nodes[s] < 0 || prev_nodes[s] < 0 || flag_rows[s] < 0)
      return shine::set_error(SHINE_E_INVALID, "shine_mesh_mark_dirty: negative count");
    if (n_nodes[s] > 0 && (!node_keys[s] || !node_ids[s] || !aligned16(node_ids[s])))
      return shine::set_error(SHINE_E_INVALID, "shine_mesh_mark_dirty: null node keys / ids (ids 16-byte aligned)");
    if (flag_rows[s] > 0 && !row_flags[s]) return shine::set_error(SHINE_E_INVALID, "shine_mesh_mark_dirty: null row flags");
    if (s <= sq && n_nodes[s] > 0 && (!sorted_keys[s] || !sorted_perm[s]))
      return shine::set_error(SHINE_E_INVALID, "shine_mesh_mark_dirty: sorted keys / permutation needed for slots <= sq");
    a.keys[s] = reinterpret_cast<const long long*>(node_keys[s]);
    a.ids[s] = node_ids[s];
    a.flags[s] = row_flags[s];
    a.sorted[s] = reinterpret_cast<const long long*>(sorted_keys[s]);
    a.perm[s] = reinterpret_cast<const long long*>(sorted_perm[s]);
    a.n[s] = n_nodes[s];
    a.prev[s] = prev_nodes[s];
    a.flag_rows[s] = flag_rows[s];
    if (s >= sq) {
      a.block0[s - sq] = (unsigned int)blocks;
      blocks += (n_nodes[s] + T - 1) / T;
      if (blocks > MAX_BLOCKS) return shine::set_error(SHINE_E_INVALID, "shine_mesh_mark_dirty: too many nodes for one launch");
    }
  }
  a.block0[n_levels - sq] = (unsigned int)blocks;
  hipStream_t st = (hipStream_t)stream;
  SHINE_HIP_CHECK(hipMemsetAsync(counts_out, 0, 2 * sizeof(int64_t), st));
  const long long nq = n_nodes[sq];
  if (nq == 0) return SHINE_OK;
  if (!dirty_out) return shine::set_error(SHINE_E_INVALID, "shine_mesh_mark_dirty: null dirty_out");
  SHINE_HIP_CHECK(hipMemsetAsync(dirty_out, 0, (size_t)nq, st));
  hipLaunchKernelGGL(k_mark_scatter, dim3((unsigned int)blocks), dim3(T), 0, st, a, dirty_out);
  SHINE_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_mark_gather, dim3((unsigned int)((nq + T - 1) / T)), dim3(T), 0, st, a, dirty_out,
                     reinterpret_cast<unsigned long long*>(counts_out));
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}

extern "C" int shine_blocks_scatter(const float* sdf, const uint8_t* mask, const int64_t* index, int64_t n, int64_t block_points,
                                    int64_t capacity, float* values, uint8_t* masks, void* stream) {
  if (n < 0 || block_points < 1 || capacity < 0 || n > MAX_BLOCKS || block_points > MAX_BLOCKS)
    return shine::set_error(SHINE_E_INVALID, "shine_blocks_scatter: bad sizes");
  if (n == 0) return SHINE_OK;
  const long long total = (long long)n * block_points;
  const long long blocks = (total + T - 1) / T;
  if (!sdf || !index || !values || !masks || blocks > MAX_BLOCKS)
    return shine::set_error(SHINE_E_INVALID, "shine_blocks_scatter: null argument or too many points for one launch");
  hipLaunchKernelGGL(k_blocks_scatter, dim3((unsigned int)blocks), dim3(T), 0, (hipStream_t)stream, sdf, mask,
                     reinterpret_cast<const long long*>(index), total, (long long)block_points, (long long)capacity, values, masks);
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}
