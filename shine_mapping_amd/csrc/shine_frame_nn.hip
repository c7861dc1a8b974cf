// shine_frame_nn.hip — neighbourhood searches over a frame's own cloud (LiDARDataset's filter_noise and estimate_normal,
// dataset/lidar_dataset.py:138-195), fp64 throughout.
//
// ONE search, three consumers.  The cloud is its own reference set: the grid is the two-level grid of shine_eval.hip (built by
// shine_eval_grid_count / shine_eval_grid_emit), whose point array is already sorted by cell, so sorted point j is query j and a
// wave's 64 lanes walk neighbouring cells.  A lane walks shells of COARSE cells outwards from its own, exactly as k_nn_search
// does, but the pruning bound is the search radius until its list holds k points and the k-th squared distance after that; the
// walk ends when that bound is below the lower bound of everything not yet visited, so the list is the exact k nearest points
// inside the radius.  The list is ordered by (squared distance, caller's index): equal distances go to the lower index.
//
//   top-k list     in LDS, one column per lane ([slot][lane]: slot t of every lane in one 64-wide row, no bank conflict between
//                  lanes), 32 slots x (8-byte distance + 4-byte sorted position) x 64 lanes = 24 KiB per one-wave workgroup.
//                  A list of 32 in registers would need dynamic indexing, i.e. scratch memory; six such workgroups fit one CU.
//                  The list starts with the k points around the query in the sorted array (mostly its own cell), so the bound
//                  is tight before the first cell is visited; the k-th distance is mirrored in a register.
//   distances      (qx - px)^2 + (qy - py)^2 + (qz - pz)^2 summed left to right with no fused multiply-add: the bits numpy's
//                  brute force produces, so "inside the radius" and the order of the list can be compared exactly.
//   widening       an unbounded search (radius < 0) runs in rounds.  Round 0 searches radius R0 = one coarse cell edge for every
//                  point; a point whose list is full is final (its k-th distance is <= R and every cell within R was visited).
//                  The others are appended to a list (an integer atomic counter; the results do not depend on the list's order)
//                  and searched again with 2 R, the host reading back one count per round, until none is left or R covers the
//                  grid's diagonal, when every remaining point is final with min(k, n) neighbours.
//   consumers      KnnOut      the lists themselves: idx [n,k] (-1 padded), d2 [n,k], count [n]
//                  MeanDistOut open3d's remove_statistical_outlier input: mean of sqrt(d2) over the neighbours found
//                  NormalOut   open3d's estimate_normals: covariance about the neighbours' mean (two passes over the list),
//                              cyclic Jacobi on the 3 x 3, eigenvector of the smallest eigenvalue, flipped towards the viewpoint
//   SOR statistics k_sor_stats: one workgroup, every thread sums a fixed strided subset, then a fixed LDS tree: the mean of the
//                  per-point means and the sum of squared deviations are the same bits on every run (no float atomics).
#include "shine_eval_grid.hpp"

namespace {

using namespace shine::grid;

constexpr int W = 64;       // one wave per workgroup, one point per lane
constexpr int KMAX = 32;    // most neighbours per point
constexpr int STAT_T = 256;
constexpr int JACOBI_SWEEPS = 8;

struct TopK {  // this lane's column of the workgroup's LDS list
  double* d2;
  int* s;
  __device__ __forceinline__ double& D(int t) const { return d2[t * W]; }
  __device__ __forceinline__ int& S(int t) const { return s[t * W]; }
};

#pragma clang fp contract(off)  // (numpy's (d * d).sum(-1) has no fused multiply-add: radius tests and ties are compared exactly)
__device__ __forceinline__ double dist2(double qx, double qy, double qz, const double* __restrict__ p) {
  const double ex = qx - p[0], ey = qy - p[1], ez = qz - p[2];
  return ex * ex + ey * ey + ez * ez;
}

// sorted point s at squared distance d2 is put into the list if it belongs among the k first in (d2, caller's index) order.
// cnt = entries held; worst = the last entry's d2 once the list is full (a register copy: most candidates are turned away by
// it without touching LDS).  -> whether the list changed
__device__ __forceinline__ bool offer(const GridDev& g, const TopK& L, int k, int s, double d2, int& cnt, double& worst) {
  if (cnt == k && (d2 > worst || (d2 == worst && g.sidx[s] > g.sidx[L.S(k - 1)]))) return false;
  int t = cnt < k ? cnt : k - 1;  // the slot that is free (or given up); larger entries move up to it
  while (t > 0) {
    const double dp = L.D(t - 1);
    if (dp < d2 || (dp == d2 && g.sidx[L.S(t - 1)] < g.sidx[s])) break;
    L.D(t) = dp;
    L.S(t) = L.S(t - 1);
    --t;
  }
  L.D(t) = d2;
  L.S(t) = s;
  if (cnt < k) ++cnt;
  if (cnt == k) worst = L.D(k - 1);
  return true;
}

// the k nearest points of sorted point j (of n) with d2 <= radius^2, ascending by (d2, caller's index), in `L`; -> how many
__device__ int knn_walk(const GridDev& g, long long n, long long j, int k, double radius, const TopK& L) {
  const double qx = g.pts[3 * j], qy = g.pts[3 * j + 1], qz = g.pts[3 * j + 2];
  const double tf[3] = {(qx - g.o.x) / g.cell, (qy - g.o.y) / g.cell, (qz - g.o.z) / g.cell};
  const double r2 = radius * radius;
  const double rc = radius / g.cell;
  const double bound0 = rc * rc * (1.0 + 0x1.0p-40);  // pruning bounds are in fine-cell units, squared
  const double inv_cell2 = 1.0 / (g.cell * g.cell);
  double bound = bound0, worst = INFINITY;
  int cnt = 0;
  // seed: the k points around j in the sorted array are mostly j's own cell, so the list is full and the bound tight before
  // the walk starts (the walk visits cells in storage order, not nearest first); the walk skips them
  long long seed_hi = j + k / 2 < n - 1 ? j + k / 2 : n - 1;
  const long long seed_lo = seed_hi - k + 1 > 0 ? seed_hi - k + 1 : 0;
  seed_hi = seed_lo + k - 1 < n - 1 ? seed_lo + k - 1 : n - 1;
  for (long long s = seed_lo; s <= seed_hi; ++s) {
    const double d2 = dist2(qx, qy, qz, g.pts + 3 * s);
    if (d2 <= r2) offer(g, L, k, (int)s, d2, cnt, worst);
  }
  if (cnt == k) bound = fmin(bound0, worst * inv_cell2 * (1.0 + 0x1.0p-40));
  long long c0[3], shells = 0;
  bool sane = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double tc = tf[a] / FINE_PER_COARSE;
    sane = sane && isfinite(tc);
    c0[a] = (long long)fmin(fmax(floor(tc), 0.0), (double)g.cmax[a]);
    const long long reach = c0[a] > g.cmax[a] - c0[a] ? c0[a] : g.cmax[a] - c0[a];
    shells = reach > shells ? reach : shells;  // beyond this shell there is no grid: the walk is bounded by the grid's extent
  }
  for (long long sh = 0; sane && sh <= shells; ++sh) {
    for (long long dx = -sh; dx <= sh; ++dx) {
      const long long cx = c0[0] + dx;
      if (cx < 0 || cx > g.cmax[0]) continue;
      const double gx = axis_gap(tf[0], (double)(cx * FINE_PER_COARSE), (double)FINE_PER_COARSE);
      if (gx * gx > bound) continue;
      for (long long dy = -sh; dy <= sh; ++dy) {
        const long long cy = c0[1] + dy;
        if (cy < 0 || cy > g.cmax[1]) continue;
        const double gy = axis_gap(tf[1], (double)(cy * FINE_PER_COARSE), (double)FINE_PER_COARSE);
        if (gx * gx + gy * gy > bound) continue;
        const bool face = dx == -sh || dx == sh || dy == -sh || dy == sh;
        const long long step = (face || sh == 0) ? 1 : 2 * sh;  // inside the shell's faces only dz = -sh and dz = sh belong to it
        for (long long dz = -sh; dz <= sh; dz += step) {
          const long long cz = c0[2] + dz;
          if (cz < 0 || cz > g.cmax[2]) continue;
          const double gz = axis_gap(tf[2], (double)(cz * FINE_PER_COARSE), (double)FINE_PER_COARSE);
          if (gx * gx + gy * gy + gz * gz > bound) continue;
          int f0, f1;
          coarse_probe(g, coarse_key(cx, cy, cz), f0, f1);
          for (int fc = f0; fc < f1; ++fc) {
            const Cell e = g.fine[fc];
            const unsigned long long local = e.key & ((1ull << LOCAL_BITS) - 1);
            const double fx = (double)(cx * FINE_PER_COARSE + (long long)(local >> (2 * FINE_BITS)));
            const double fy = (double)(cy * FINE_PER_COARSE + (long long)((local >> FINE_BITS) & (FINE_PER_COARSE - 1)));
            const double fz = (double)(cz * FINE_PER_COARSE + (long long)(local & (FINE_PER_COARSE - 1)));
            const double hx = axis_gap(tf[0], fx, 1.0), hy = axis_gap(tf[1], fy, 1.0), hz = axis_gap(tf[2], fz, 1.0);
            if (hx * hx + hy * hy + hz * hz > bound) continue;
            for (int s = e.first; s < e.end; ++s) {
              if (s >= seed_lo && s <= seed_hi) continue;
              const double d2 = dist2(qx, qy, qz, g.pts + 3ll * s);
              if (d2 <= r2 && offer(g, L, k, s, d2, cnt, worst) && cnt == k)
                bound = fmin(bound0, worst * inv_cell2 * (1.0 + 0x1.0p-40));
            }
          }
        }
      }
    }
    // lower bound (fine-cell units) of everything outside the block of shells 0..sh: the nearest of its faces that still has
    // grid beyond it
    double lb = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (c0[a] - sh > 0) lb = fmin(lb, fmax(tf[a] - (double)((c0[a] - sh) * FINE_PER_COARSE) - MARGIN, 0.0));
      if (c0[a] + sh < g.cmax[a]) lb = fmin(lb, fmax((double)((c0[a] + sh + 1) * FINE_PER_COARSE) - MARGIN - tf[a], 0.0));
    }
    if (!(lb * lb <= bound)) break;
  }
  return cnt;
}

// ---------------------------------------------------------------- the three consumers
struct KnnOut {
  int* idx;      // [n][k]
  double* d2;    // [n][k]
  int* count;    // [n]
  __device__ void operator()(const GridDev& g, long long j, int k, int cnt, const TopK& L) const {
    const long long i = g.sidx[j];
    for (int t = 0; t < k; ++t) {
      idx[i * k + t] = t < cnt ? g.sidx[L.S(t)] : -1;
      d2[i * k + t] = t < cnt ? L.D(t) : INFINITY;
    }
    count[i] = cnt;
  }
};

struct MeanDistOut {
  double* mean;  // [n]
  __device__ void operator()(const GridDev& g, long long j, int, int cnt, const TopK& L) const {
    double sum = 0.0;
    for (int t = 0; t < cnt; ++t) sum += sqrt(L.D(t));  // ascending: the same order on every run
    mean[g.sidx[j]] = cnt > 0 ? sum / (double)cnt : 0.0;
  }
};

// one Jacobi rotation that zeroes a[p][q] of the symmetric 3 x 3 (r = the third index), accumulated into the columns of v
__device__ __forceinline__ void jacobi_rotate(double (&a)[3][3], double (&v)[3][3], int p, int q, int r) {
  const double apq = a[p][q];
  if (apq == 0.0) return;
  const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));  // the smaller root: |angle| <= pi/4
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  a[p][p] -= t * apq;
  a[q][q] += t * apq;
  a[p][q] = a[q][p] = 0.0;
  const double arp = a[r][p], arq = a[r][q];
  a[r][p] = a[p][r] = c * arp - s * arq;
  a[r][q] = a[q][r] = s * arp + c * arq;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double vip = v[i][p], viq = v[i][q];
    v[i][p] = c * vip - s * viq;
    v[i][q] = s * vip + c * viq;
  }
}

struct NormalOut {
  double* normals;  // [n][3]
  Vec3 view;
  __device__ void operator()(const GridDev& g, long long j, int, int cnt, const TopK& L) const {
    const double px = g.pts[3 * j], py = g.pts[3 * j + 1], pz = g.pts[3 * j + 2];
    double n[3] = {0.0, 0.0, 1.0};  // open3d's fallback: fewer than 3 neighbours, or no direction at all
    if (cnt >= 3) {
      double m[3] = {0.0, 0.0, 0.0};
      for (int t = 0; t < cnt; ++t) {
        const double* q = g.pts + 3ll * L.S(t);
        m[0] += q[0];
        m[1] += q[1];
        m[2] += q[2];
      }
      m[0] /= (double)cnt;
      m[1] /= (double)cnt;
      m[2] /= (double)cnt;
      // centred before accumulating: coordinates reach tens of metres, neighbourhoods are decimetres
      double a[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
      for (int t = 0; t < cnt; ++t) {
        const double* q = g.pts + 3ll * L.S(t);
        const double x = q[0] - m[0], y = q[1] - m[1], z = q[2] - m[2];
        a[0][0] += x * x;
        a[0][1] += x * y;
        a[0][2] += x * z;
        a[1][1] += y * y;
        a[1][2] += y * z;
        a[2][2] += z * z;
      }
      a[1][0] = a[0][1];
      a[2][0] = a[0][2];
      a[2][1] = a[1][2];
      if (a[0][0] + a[1][1] + a[2][2] > 0.0) {  // (all neighbours in one place: no direction, the fallback stays)
        double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
        for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {  // cyclic Jacobi: backward stable, quadratic convergence
          jacobi_rotate(a, v, 0, 1, 2);
          jacobi_rotate(a, v, 0, 2, 1);
          jacobi_rotate(a, v, 1, 2, 0);
        }
        // the column of the smallest eigenvalue (the first of equal ones), picked without indexing by a variable
        const bool c1 = a[1][1] < a[0][0];
        const double lo01 = c1 ? a[1][1] : a[0][0];
        const bool c2 = a[2][2] < lo01;
        const double e0 = c2 ? v[0][2] : c1 ? v[0][1] : v[0][0];
        const double e1 = c2 ? v[1][2] : c1 ? v[1][1] : v[1][0];
        const double e2 = c2 ? v[2][2] : c1 ? v[2][1] : v[2][0];
        const double len = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
        if (len > 0.0 && isfinite(len)) {
          n[0] = e0 / len;
          n[1] = e1 / len;
          n[2] = e2 / len;
        }
      }
    }
    // towards the viewpoint: n . (viewpoint - p) >= 0
    if (n[0] * (view.x - px) + n[1] * (view.y - py) + n[2] * (view.z - pz) < 0.0) {
      n[0] = -n[0];
      n[1] = -n[1];
      n[2] = -n[2];
    }
    const long long i = g.sidx[j];
    normals[3 * i] = n[0];
    normals[3 * i + 1] = n[1];
    normals[3 * i + 2] = n[2];
  }
};

// one lane per point.  active == nullptr: sorted points 0..n_active-1, else the listed ones.  A point of an unbounded search
// (next != nullptr) whose list is not full is not final: it is appended to `next` for the round with twice the radius.
template <class Consumer>
__global__ __launch_bounds__(W) void k_frame_nn(GridDev g, long long n, const int* __restrict__ active, long long n_active, int k,
                                                double radius, int* __restrict__ next, int* __restrict__ next_count, Consumer out) {
  __shared__ double s_d2[KMAX * W];
  __shared__ int s_pos[KMAX * W];
  const long long a = (long long)blockIdx.x * W + threadIdx.x;
  if (a >= n_active) return;
  const long long j = active ? (long long)active[a] : a;
  const TopK L{s_d2 + threadIdx.x, s_pos + threadIdx.x};
  const int cnt = knn_walk(g, n, j, k, radius, L);
  if (next && cnt < k) {
    next[atomicAdd(next_count, 1)] = (int)j;
    return;
  }
  out(g, j, k, cnt, L);
}

// {mean of v, sum of (v - mean)^2} in a fixed order: thread t adds v[t], v[t + 256], ...; the 256 partial sums meet in a tree
__global__ __launch_bounds__(STAT_T) void k_sor_stats(const double* __restrict__ v, long long n, double* __restrict__ out) {
  __shared__ double s[STAT_T];
  __shared__ double s_mean;
  for (int pass = 0; pass < 2; ++pass) {
    const double mean = pass ? s_mean : 0.0;
    double acc = 0.0;
    for (long long i = threadIdx.x; i < n; i += STAT_T) {
      const double d = v[i] - mean;
      acc += pass ? d * d : d;
    }
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int o = STAT_T / 2; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      if (pass == 0) s_mean = s[0] / (double)n;
      out[pass] = pass ? s[0] : s[0] / (double)n;
    }
    __syncthreads();
  }
}

struct NnScratch {
  int *list0, *list1, *count;
  size_t bytes;
};

NnScratch nn_scratch(void* ws, long long n) {
  shine::Arena c(ws);
  NnScratch s;
  s.list0 = c.take<int>((size_t)n);
  s.list1 = c.take<int>((size_t)n);
  s.count = c.take<int>(1);
  s.bytes = c.bytes();
  return s;
}

unsigned blocks_of(long long n) { return (unsigned)((n + W - 1) / W); }

// a radius that holds the whole grid (hence the whole cloud): its diagonal, rounded up
double grid_diagonal(const int64_t* cells_per_axis, double cell) {
  double s = 0.0;
  for (int a = 0; a < 3; ++a) {
    const double e = (double)cells_per_axis[a] * cell;
    s += e * e;
  }
  return sqrt(s) * (1.0 + 0x1.0p-20);
}

// the search of every point, bounded (radius >= 0: one launch) or unbounded (radius < 0: the widening rounds)
template <class Consumer>
int run_search(const GridDev& g, long long n, const int64_t* cells_per_axis, int k, double radius, const NnScratch& s,
               hipStream_t st, const Consumer& out, int32_t* rounds_out) {
  if (radius >= 0.0) {
    hipLaunchKernelGGL(k_frame_nn<Consumer>, dim3(blocks_of(n)), dim3(W), 0, st, g, n, (const int*)nullptr, n, k, radius,
                       (int*)nullptr, (int*)nullptr, out);
    SHINE_HIP_CHECK(hipGetLastError());
    if (rounds_out) *rounds_out = 1;
    return SHINE_OK;
  }
  const double diag = grid_diagonal(cells_per_axis, g.cell);
  double r = g.cell * FINE_PER_COARSE;
  if (n <= k) r = diag;  // (no list can fill: every point needs the whole cloud)
  const int* active = nullptr;
  int* lists[2] = {s.list0, s.list1};
  long long n_active = n;
  int rounds = 0;
  while (n_active > 0) {
    const bool last = r >= diag;
    ++rounds;
    if (!last) SHINE_HIP_CHECK(hipMemsetAsync(s.count, 0, 4, st));
    hipLaunchKernelGGL(k_frame_nn<Consumer>, dim3(blocks_of(n_active)), dim3(W), 0, st, g, n, active, n_active, k, last ? diag : r,
                       last ? (int*)nullptr : lists[rounds & 1], last ? (int*)nullptr : s.count, out);
    SHINE_HIP_CHECK(hipGetLastError());
    if (last) break;
    int left = 0;
    SHINE_HIP_CHECK(hipMemcpyAsync(&left, s.count, 4, hipMemcpyDeviceToHost, st));
    SHINE_HIP_CHECK(hipStreamSynchronize(st));
    active = lists[rounds & 1];
    n_active = left;
    r *= 2.0;
  }
  if (rounds_out) *rounds_out = rounds;
  return SHINE_OK;
}

// the argument checks the three entry points share; -> SHINE_OK and the grid view
int check_grid(const char* who, const void* grid, int64_t n, int64_t n_fine, int64_t n_coarse, const double* origin, double cell,
               const int64_t* cells_per_axis, GridDev* g) {
  char msg[160];
  if (!grid || !origin || !cells_per_axis || !(cell > 0.0)) {
    snprintf(msg, sizeof msg, "%s: null argument or cell <= 0", who);
    return shine::set_error(SHINE_E_INVALID, msg);
  }
  if (!grid_dev(grid, n, n_fine, n_coarse, origin, cell, cells_per_axis, g)) {
    snprintf(msg, sizeof msg, "%s: cells_per_axis out of range (1 .. 2^21)", who);
    return shine::set_error(SHINE_E_INVALID, msg);
  }
  return SHINE_OK;
}

int check_sizes(const char* who, const char* k_name, int64_t n, int64_t n_fine, int64_t n_coarse, int32_t k, const size_t* workspace_bytes) {
  char msg[160];
  if (!workspace_bytes || bad_count(n) || n == 0 || n_fine < 1 || n_fine > n || n_coarse < 1 || n_coarse > n_fine) {
    snprintf(msg, sizeof msg, "%s: bad sizes (0 < n < 2^31, 1 <= n_coarse <= n_fine <= n)", who);
    return shine::set_error(SHINE_E_INVALID, msg);
  }
  if (k < 1 || k > KMAX) {
    snprintf(msg, sizeof msg, "%s: %s must be 1..32", who, k_name);
    return shine::set_error(SHINE_E_INVALID, msg);
  }
  return SHINE_OK;
}

}  // namespace

extern "C" int shine_knn_search(const void* grid, int64_t n, int64_t n_fine, int64_t n_coarse, const double* origin, double cell,
                                const int64_t* cells_per_axis, int32_t k, double radius, void* workspace, size_t* workspace_bytes,
                                int32_t* idx_out, double* d2_out, int32_t* count_out, int32_t* rounds_out, void* stream) {
  if (int rc = check_sizes("shine_knn_search", "k", n, n_fine, n_coarse, k, workspace_bytes)) return rc;
  const NnScratch s = nn_scratch(workspace, n);
  SHINE_WORKSPACE_GATE(s.bytes, workspace, workspace_bytes, "shine_knn_search");
  if (!idx_out || !d2_out || !count_out || radius != radius)
    return shine::set_error(SHINE_E_INVALID, "shine_knn_search: null argument or radius is NaN");
  GridDev g;
  if (int rc = check_grid("shine_knn_search", grid, n, n_fine, n_coarse, origin, cell, cells_per_axis, &g)) return rc;
  return run_search(g, n, cells_per_axis, k, radius, s, (hipStream_t)stream, KnnOut{idx_out, d2_out, count_out}, rounds_out);
}

extern "C" int shine_sor_mean_dist(const void* grid, int64_t n, int64_t n_fine, int64_t n_coarse, const double* origin, double cell,
                                   const int64_t* cells_per_axis, int32_t k, void* workspace, size_t* workspace_bytes,
                                   double* mean_dist_out, double* stats_out, int32_t* rounds_out, void* stream) {
  if (int rc = check_sizes("shine_sor_mean_dist", "k", n, n_fine, n_coarse, k, workspace_bytes)) return rc;
  const NnScratch s = nn_scratch(workspace, n);
  SHINE_WORKSPACE_GATE(s.bytes, workspace, workspace_bytes, "shine_sor_mean_dist");
  if (!mean_dist_out || !stats_out) return shine::set_error(SHINE_E_INVALID, "shine_sor_mean_dist: null argument");
  GridDev g;
  if (int rc = check_grid("shine_sor_mean_dist", grid, n, n_fine, n_coarse, origin, cell, cells_per_axis, &g)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = run_search(g, n, cells_per_axis, k, -1.0, s, st, MeanDistOut{mean_dist_out}, rounds_out)) return rc;
  hipLaunchKernelGGL(k_sor_stats, dim3(1), dim3(STAT_T), 0, st, (const double*)mean_dist_out, (long long)n, stats_out);
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}

extern "C" int shine_frame_normals(const void* grid, int64_t n, int64_t n_fine, int64_t n_coarse, const double* origin, double cell,
                                   const int64_t* cells_per_axis, double radius, int32_t max_nn, const double* viewpoint,
                                   void* workspace, size_t* workspace_bytes, double* normals_out, void* stream) {
  if (int rc = check_sizes("shine_frame_normals", "max_nn", n, n_fine, n_coarse, max_nn, workspace_bytes)) return rc;
  const NnScratch s = nn_scratch(workspace, n);
  SHINE_WORKSPACE_GATE(s.bytes, workspace, workspace_bytes, "shine_frame_normals");
  if (!normals_out || !viewpoint || !(radius >= 0.0) || radius == INFINITY)
    return shine::set_error(SHINE_E_INVALID, "shine_frame_normals: null argument or radius not a finite number >= 0");
  GridDev g;
  if (int rc = check_grid("shine_frame_normals", grid, n, n_fine, n_coarse, origin, cell, cells_per_axis, &g)) return rc;
  const NormalOut out{normals_out, Vec3{viewpoint[0], viewpoint[1], viewpoint[2]}};
  return run_search(g, n, cells_per_axis, max_nn, radius, s, (hipStream_t)stream, out, nullptr);
}
