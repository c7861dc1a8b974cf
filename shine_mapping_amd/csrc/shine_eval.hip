// shine_eval.hip — mesh evaluation on the device (eval/eval_utils.py: eval_mesh, nn_correspondance, crop_intersection), fp64
// geometry throughout.  Stages, each its own entry point:
//   bounds / box mask   per-axis min and max of a cloud; which points lie inside an inclusive box (the crop of the mesh)
//   sample              uniform points on a mesh: fp64 areas, a deterministic three-launch inclusive scan, one binary search
//                       and one barycentric point per sample; uniforms from a counter-based generator of (seed, sample, j)
//   voxel down-sample   64-bit voxel keys (21 bits per axis), a stable radix sort of (key, index), one thread per occupied
//                       voxel summing its run in index order: the mean is the same bits every run
//   nearest neighbour   a two-level uniform grid over the reference set.  Fine cells (edge h) are grouped 4 x 4 x 4 into
//                       coarse cells (edge C = 4 h); the points are sorted by (coarse cell, fine cell), every occupied fine
//                       cell is one 16-byte entry {key, first point, end point}, the fine cells of one coarse cell are
//                       contiguous, and the occupied coarse cells sit in an open-addressing table of 16-byte entries {key,
//                       first fine cell, end fine cell}.  One query per lane walks shells of COARSE cells outwards from its
//                       own: a coarse cell is probed only if its box is nearer than the best distance so far (and nearer
//                       than the truncation), the fine cells of an occupied one are box-tested the same way before their
//                       points are read.  The walk stops when the best distance is within the lower bound of everything not
//                       yet visited or that bound reaches the truncation.  A query with nothing nearby therefore costs at most
//                       (2 ceil(truncation / C) + 1)^3 probes of a small table and never looks at an empty fine cell.
//                       Queries are sorted by their cell so that a wave's lanes walk the same cells; results are written in the
//                       caller's order.  Every box is widened by 2^-20 of a cell, far above the rounding of the cell
//                       assignment, so pruning never hides the exact nearest point; distances are computed from the
//                       original fp64 coordinates.
//   metrics             one launch: the sums, sums of squares and below-threshold counts of the two distance arrays (fixed
//                       partition into blocks, the last block to arrive — shine_arrive.hpp — adds the partials in block order).
#include "shine_arrive.hpp"
#include "shine_eval_grid.hpp"

namespace {

using namespace shine::grid;  // the grid's constants, layout and cell arithmetic (shared with shine_frame_nn.hip)

constexpr int T = 256;
constexpr int RED_BLOCKS = 256;                  // blocks of the bounds / metrics reductions

unsigned grid_of(long long n) { return (unsigned)((n + T - 1) / T); }

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// ---------------------------------------------------------------- bounds, box mask
__global__ void k_bounds_partial(const double* __restrict__ p, long long n, double* __restrict__ part) {
  __shared__ double s[6][T];
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (long long i = (long long)blockIdx.x * T + threadIdx.x; i < n; i += (long long)gridDim.x * T)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double v = p[3 * i + a];
      lo[a] = fmin(lo[a], v);
      hi[a] = fmax(hi[a], v);
    }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    s[a][threadIdx.x] = lo[a];
    s[3 + a][threadIdx.x] = hi[a];
  }
  __syncthreads();
  for (int o = T / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        s[a][threadIdx.x] = fmin(s[a][threadIdx.x], s[a][threadIdx.x + o]);
        s[3 + a][threadIdx.x] = fmax(s[3 + a][threadIdx.x], s[3 + a][threadIdx.x + o]);
      }
    __syncthreads();
  }
  if (threadIdx.x < 6) part[6 * blockIdx.x + threadIdx.x] = s[threadIdx.x][0];
}

__global__ void k_bounds_final(const double* __restrict__ part, int blocks, double* __restrict__ out) {
  const int a = threadIdx.x;
  if (a >= 6) return;
  double v = part[a];
  for (int b = 1; b < blocks; ++b) v = a < 3 ? fmin(v, part[6 * b + a]) : fmax(v, part[6 * b + a]);
  out[a] = v;
}

__global__ void k_outside_box(const double* __restrict__ p, long long n, Vec3 lo, Vec3 hi, unsigned char* __restrict__ drop) {
  const long long i = (long long)blockIdx.x * T + threadIdx.x;
  if (i >= n) return;
  const double x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
  const bool in = x >= lo.x && x <= hi.x && y >= lo.y && y <= hi.y && z >= lo.z && z <= hi.z;
  drop[i] = in ? 0 : 1;
}

// ---------------------------------------------------------------- mesh sampling
__device__ __forceinline__ double tri_area(const double* __restrict__ v, const int* __restrict__ f, long long t) {
  const long long a = f[3 * t], b = f[3 * t + 1], c = f[3 * t + 2];
  const double e1x = v[3 * b] - v[3 * a], e1y = v[3 * b + 1] - v[3 * a + 1], e1z = v[3 * b + 2] - v[3 * a + 2];
  const double e2x = v[3 * c] - v[3 * a], e2y = v[3 * c + 1] - v[3 * a + 1], e2z = v[3 * c + 2] - v[3 * a + 2];
  const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  return 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
}

// inclusive scan of the areas in three launches with a fixed summation order: each block scans 1024 areas (4 per thread),
// one thread adds the block totals up in block order, every block adds its offset
__global__ void k_area_scan_block(const double* __restrict__ v, const int* __restrict__ f, long long nf, long long nv,
                                  double* __restrict__ cum, double* __restrict__ block_tot) {
  __shared__ double s[T];
  const long long t0 = ((long long)blockIdx.x * T + threadIdx.x) * 4;
  double a[4];
  double run = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double ar = 0.0;
    if (t0 + j < nf) {
      const long long t = t0 + j;
      const int i0 = f[3 * t], i1 = f[3 * t + 1], i2 = f[3 * t + 2];
      if (i0 >= 0 && i1 >= 0 && i2 >= 0 && i0 < nv && i1 < nv && i2 < nv) ar = tri_area(v, f, t);  // (a bad id has no area)
    }
    run += ar;
    a[j] = run;
  }
  s[threadIdx.x] = run;
  __syncthreads();
  for (int o = 1; o < T; o <<= 1) {
    const double add = (int)threadIdx.x >= o ? s[threadIdx.x - o] : 0.0;
    __syncthreads();
    s[threadIdx.x] += add;
    __syncthreads();
  }
  const double before = threadIdx.x ? s[threadIdx.x - 1] : 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (t0 + j < nf) cum[t0 + j] = before + a[j];
  if (threadIdx.x == T - 1) block_tot[blockIdx.x] = s[T - 1];
}

__global__ void k_area_scan_totals(double* __restrict__ block_tot, int blocks) {
  if (blockIdx.x || threadIdx.x) return;
  double run = 0.0;
  for (int b = 0; b < blocks; ++b) {  // exclusive, in block order
    const double t = block_tot[b];
    block_tot[b] = run;
    run += t;
  }
}

__global__ void k_area_scan_add(double* __restrict__ cum, const double* __restrict__ block_tot, long long nf) {
  const long long t = (long long)blockIdx.x * T + threadIdx.x;
  if (t < nf) cum[t] += block_tot[t / (4 * T)];
}

__global__ void k_sample(const double* __restrict__ v, const int* __restrict__ f, long long nf, const double* __restrict__ cum,
                         long long n, unsigned long long seed, const double* __restrict__ uniforms, double* __restrict__ out,
                         int* __restrict__ tri_out) {
  const long long i = (long long)blockIdx.x * T + threadIdx.x;
  if (i >= n) return;
  double u[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
    u[j] = uniforms ? uniforms[3 * i + j]
                    : (double)(mix64(seed + 0x9E3779B97F4A7C15ull * (3ull * (unsigned long long)i + j + 1)) >> 11) * 0x1.0p-53;
  const double total = cum[nf - 1];
  // first triangle whose cumulative share is > u0 (a zero-area triangle repeats its predecessor's share: never the first)
  long long lo = 0, hi = nf - 1;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (cum[mid] / total > u[0]) hi = mid;
    else lo = mid + 1;
  }
  const long long a = f[3 * lo], b = f[3 * lo + 1], c = f[3 * lo + 2];
  const double r = sqrt(u[1]);
  const double w0 = 1.0 - r, w1 = r * (1.0 - u[2]), w2 = r * u[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) out[3 * i + k] = w0 * v[3 * a + k] + w1 * v[3 * b + k] + w2 * v[3 * c + k];
  if (tri_out) tri_out[i] = (int)lo;
}

// ---------------------------------------------------------------- voxel down-sampling
__device__ __forceinline__ long long cell_of(double p, double origin, double cell) {
  const double t = floor((p - origin) / cell);
  return (long long)fmin(fmax(t, 0.0), (double)AXIS_MAX);  // (NaN and out-of-range points land in a border cell)
}

__global__ void k_voxel_keys(const double* __restrict__ p, long long n, Vec3 o, double voxel, unsigned long long* __restrict__ keys,
                             unsigned long long* __restrict__ vals) {
  const long long i = (long long)blockIdx.x * T + threadIdx.x;
  if (i >= n) return;
  const unsigned long long x = cell_of(p[3 * i], o.x, voxel), y = cell_of(p[3 * i + 1], o.y, voxel), z = cell_of(p[3 * i + 2], o.z, voxel);
  keys[i] = (x << 42) | (y << 21) | z;
  vals[i] = (unsigned long long)i;
}

__global__ void k_run_flags(const unsigned long long* __restrict__ keys, long long n, int shift, unsigned char* __restrict__ flags) {
  const long long j = (long long)blockIdx.x * T + threadIdx.x;
  if (j < n) flags[j] = (j == 0 || (keys[j] >> shift) != (keys[j - 1] >> shift)) ? 1 : 0;
}

__global__ void k_voxel_mean(const double* __restrict__ p, const unsigned long long* __restrict__ keys,
                             const unsigned long long* __restrict__ vals, const unsigned char* __restrict__ flags,
                             const int* __restrict__ rank, long long n, double* __restrict__ out,
                             unsigned long long* __restrict__ keys_out) {
  const long long j = (long long)blockIdx.x * T + threadIdx.x;
  if (j >= n || !flags[j]) return;
  double x = 0.0, y = 0.0, z = 0.0;
  long long e = j;
  do {  // the sort is stable: the run is in the caller's point order
    const long long i = (long long)vals[e];
    x += p[3 * i];
    y += p[3 * i + 1];
    z += p[3 * i + 2];
    ++e;
  } while (e < n && !flags[e]);
  const double c = (double)(e - j);
  const long long o = rank[j];
  out[3 * o] = x / c;
  out[3 * o + 1] = y / c;
  out[3 * o + 2] = z / c;
  if (keys_out) keys_out[o] = keys[j];
}

constexpr int MAX_ATTR = 4;

// k_voxel_mean with n_attr (1..MAX_ATTR) fp64 attribute columns carried along: the same point sums in the same order (the point
// means are k_voxel_mean's bits), and per column the sum over the run in the caller's point order, divided by the count
__global__ void k_voxel_mean_attr(const double* __restrict__ p, const double* __restrict__ attrs, int n_attr,
                                  const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ vals,
                                  const unsigned char* __restrict__ flags, const int* __restrict__ rank, long long n,
                                  double* __restrict__ out, double* __restrict__ attrs_out,
                                  unsigned long long* __restrict__ keys_out) {
  const long long j = (long long)blockIdx.x * T + threadIdx.x;
  if (j >= n || !flags[j]) return;
  double x = 0.0, y = 0.0, z = 0.0;
  double a[MAX_ATTR] = {0.0, 0.0, 0.0, 0.0};
  long long e = j;
  do {
    const long long i = (long long)vals[e];
    x += p[3 * i];
    y += p[3 * i + 1];
    z += p[3 * i + 2];
#pragma unroll
    for (int k = 0; k < MAX_ATTR; ++k)
      if (k < n_attr) a[k] += attrs[i * n_attr + k];
    ++e;
  } while (e < n && !flags[e]);
  const double c = (double)(e - j);
  const long long o = rank[j];
  out[3 * o] = x / c;
  out[3 * o + 1] = y / c;
  out[3 * o + 2] = z / c;
#pragma unroll
  for (int k = 0; k < MAX_ATTR; ++k)
    if (k < n_attr) attrs_out[o * n_attr + k] = a[k] / c;
  if (keys_out) keys_out[o] = keys[j];
}

// ---------------------------------------------------------------- nearest neighbour: the grid
__global__ void k_grid_keys(const double* __restrict__ p, long long n, Vec3 o, double cell, unsigned long long* __restrict__ keys,
                            unsigned long long* __restrict__ vals) {
  const long long i = (long long)blockIdx.x * T + threadIdx.x;
  if (i >= n) return;
  keys[i] = grid_key(cell_of(p[3 * i], o.x, cell), cell_of(p[3 * i + 1], o.y, cell), cell_of(p[3 * i + 2], o.z, cell));
  vals[i] = (unsigned long long)i;
}

// one thread per sorted reference point: its coordinates and index in sorted order, and the entries its run starts / ends
__global__ void k_grid_emit(const double* __restrict__ p, const unsigned long long* __restrict__ keys,
                            const unsigned long long* __restrict__ vals, const unsigned char* __restrict__ fflag,
                            const unsigned char* __restrict__ cflag, const int* __restrict__ frank, const int* __restrict__ crank,
                            long long n, double* __restrict__ pts, int* __restrict__ sidx, Cell* __restrict__ fine,
                            Cell* __restrict__ coarse) {
  const long long j = (long long)blockIdx.x * T + threadIdx.x;
  if (j >= n) return;
  const long long i = (long long)vals[j];
  pts[3 * j] = p[3 * i];
  pts[3 * j + 1] = p[3 * i + 1];
  pts[3 * j + 2] = p[3 * i + 2];
  sidx[j] = (int)i;
  const unsigned long long key = keys[j];
  const int fr = frank[j] + fflag[j] - 1, cr = crank[j] + cflag[j] - 1;  // the fine / coarse cell this point is in
  if (fflag[j]) {
    fine[fr].key = key;
    fine[fr].first = (int)j;
  }
  const bool last = j == n - 1;
  if (last || fflag[j + 1]) fine[fr].end = (int)(j + 1);
  if (cflag[j]) {
    coarse[cr].key = key >> LOCAL_BITS;
    coarse[cr].first = fr;
  }
  if (last || cflag[j + 1]) coarse[cr].end = fr + 1;
}

__global__ void k_coarse_insert(const Cell* __restrict__ coarse, long long n_coarse, Cell* table, unsigned int shift,
                                unsigned int mask) {
  const long long c = (long long)blockIdx.x * T + threadIdx.x;
  if (c >= n_coarse) return;
  const Cell e = coarse[c];
  unsigned int slot = coarse_slot(e.key, shift);
  for (unsigned int tries = 0; tries <= mask; ++tries) {  // (the table is at most half full: a free slot exists)
    const unsigned long long old = atomicCAS(&table[slot].key, EMPTY, e.key);
    if (old == EMPTY) {
      table[slot].first = e.first;
      table[slot].end = e.end;
      return;
    }
    slot = (slot + 1) & mask;
  }
}

__global__ void k_query_keys(const double* __restrict__ q, long long n, Vec3 o, double cell, unsigned long long* __restrict__ keys,
                             unsigned long long* __restrict__ vals) {
  const long long i = (long long)blockIdx.x * T + threadIdx.x;
  if (i >= n) return;
  keys[i] = grid_key(cell_of(q[3 * i], o.x, cell), cell_of(q[3 * i + 1], o.y, cell), cell_of(q[3 * i + 2], o.z, cell));
  vals[i] = (unsigned long long)i;
}

__global__ __launch_bounds__(T) void k_nn_search(GridDev g, const double* __restrict__ q, const unsigned long long* __restrict__ order,
                                                 long long n_q, double truncation, int* __restrict__ idx_out,
                                                 double* __restrict__ dist_out, unsigned char* __restrict__ keep_out,
                                                 int* __restrict__ stats) {
  const long long j = (long long)blockIdx.x * T + threadIdx.x;
  if (j >= n_q) return;
  const long long qi = (long long)order[j];
  const double qx = q[3 * qi], qy = q[3 * qi + 1], qz = q[3 * qi + 2];
  // the query in fine-cell units and in coarse-cell units, relative to the grid's origin
  const double tf[3] = {(qx - g.o.x) / g.cell, (qy - g.o.y) / g.cell, (qz - g.o.z) / g.cell};
  const double tc[3] = {tf[0] / FINE_PER_COARSE, tf[1] / FINE_PER_COARSE, tf[2] / FINE_PER_COARSE};
  const double trunc_cells = truncation / g.cell;
  const double bound0 = trunc_cells * trunc_cells;   // pruning bounds are in fine-cell units, squared
  const double trunc2 = truncation * truncation;
  double best = trunc2;                               // squared distance in metres of the best point so far (strict <)
  double best_cells = bound0;
  int bidx = -1;
  int n_coarse_seen = 0, n_fine_seen = 0;
  long long c0[3];
  bool sane = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    sane = sane && isfinite(tc[a]);
    const double f = floor(tc[a]);
    c0[a] = (long long)fmin(fmax(f, 0.0), (double)g.cmax[a]);  // the walk starts at the grid cell nearest to the query
  }
  for (long long k = 0; sane; ++k) {
    for (long long dx = -k; dx <= k; ++dx) {
      const long long cx = c0[0] + dx;
      if (cx < 0 || cx > g.cmax[0]) continue;
      const double gx = axis_gap(tf[0], (double)(cx * FINE_PER_COARSE), (double)FINE_PER_COARSE);
      if (gx * gx > best_cells) continue;
      for (long long dy = -k; dy <= k; ++dy) {
        const long long cy = c0[1] + dy;
        if (cy < 0 || cy > g.cmax[1]) continue;
        const double gy = axis_gap(tf[1], (double)(cy * FINE_PER_COARSE), (double)FINE_PER_COARSE);
        if (gx * gx + gy * gy > best_cells) continue;
        const bool face = dx == -k || dx == k || dy == -k || dy == k;
        const long long step = (face || k == 0) ? 1 : 2 * k;  // inside the shell's faces only dz = -k and dz = k belong to it
        for (long long dz = -k; dz <= k; dz += step) {
          const long long cz = c0[2] + dz;
          if (cz < 0 || cz > g.cmax[2]) continue;
          const double gz = axis_gap(tf[2], (double)(cz * FINE_PER_COARSE), (double)FINE_PER_COARSE);
          if (gx * gx + gy * gy + gz * gz > best_cells) continue;
          // probe the coarse table
          ++n_coarse_seen;
          const unsigned long long ck = coarse_key(cx, cy, cz);
          unsigned int slot = coarse_slot(ck, g.shift);
          int f0 = 0, f1 = 0;
          for (unsigned int tries = 0; tries <= g.mask; ++tries) {
            const Cell e = g.table[slot];
            if (e.key == ck) {
              f0 = e.first;
              f1 = e.end;
              break;
            }
            if (e.key == EMPTY) break;
            slot = (slot + 1) & g.mask;
          }
          for (int fc = f0; fc < f1; ++fc) {
            const Cell e = g.fine[fc];
            ++n_fine_seen;
            const unsigned long long local = e.key & ((1ull << LOCAL_BITS) - 1);
            const double fx = (double)(cx * FINE_PER_COARSE + (long long)(local >> (2 * FINE_BITS)));
            const double fy = (double)(cy * FINE_PER_COARSE + (long long)((local >> FINE_BITS) & (FINE_PER_COARSE - 1)));
            const double fz = (double)(cz * FINE_PER_COARSE + (long long)(local & (FINE_PER_COARSE - 1)));
            const double hx = axis_gap(tf[0], fx, 1.0), hy = axis_gap(tf[1], fy, 1.0), hz = axis_gap(tf[2], fz, 1.0);
            if (hx * hx + hy * hy + hz * hz > best_cells) continue;
            for (int s = e.first; s < e.end; ++s) {
              const double ex = qx - g.pts[3ll * s], ey = qy - g.pts[3ll * s + 1], ez = qz - g.pts[3ll * s + 2];
              const double d2 = ex * ex + ey * ey + ez * ez;
              if (d2 > best) continue;
              const int si = g.sidx[s];
              if (d2 < best || (bidx >= 0 && si < bidx)) {  // ties go to the smaller index, as a brute-force argmin does
                best = d2;
                bidx = si;
                best_cells = fmin(bound0, d2 / (g.cell * g.cell) * (1.0 + 0x1.0p-40));
              }
            }
          }
        }
      }
    }
    // lower bound (fine-cell units) of everything outside the block of shells 0..k: the nearest of its faces that still
    // has grid beyond it
    double lb = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (c0[a] - k > 0) lb = fmin(lb, fmax(tf[a] - (double)((c0[a] - k) * FINE_PER_COARSE) - MARGIN, 0.0));
      if (c0[a] + k < g.cmax[a]) lb = fmin(lb, fmax((double)((c0[a] + k + 1) * FINE_PER_COARSE) - MARGIN - tf[a], 0.0));
    }
    if (!(lb * lb <= best_cells)) break;  // (also when nothing is left: lb = inf)
  }
  idx_out[qi] = bidx;
  dist_out[qi] = bidx >= 0 ? sqrt(best) : truncation;
  keep_out[qi] = bidx >= 0 ? 1 : 0;
  if (stats) {  // diagnostic mode: the largest counts of any query (the plain read only filters: the maxima never decrease)
    if (n_coarse_seen > stats[0]) atomicMax(stats, n_coarse_seen);
    if (n_fine_seen > stats[1]) atomicMax(stats + 1, n_fine_seen);
  }
}

// ---------------------------------------------------------------- metrics
struct MetricShared {
  double v[6][T / 64];
};

__global__ __launch_bounds__(T) void k_metrics(const double* __restrict__ dp, long long np, const double* __restrict__ dr,
                                               long long nr, double threshold, double* __restrict__ part,
                                               unsigned int* __restrict__ done, double* __restrict__ out) {
  __shared__ MetricShared sm;
  __shared__ unsigned is_last;
  double acc[6] = {0, 0, 0, 0, 0, 0};  // sum p, sum p^2, count p < thr, sum r, sum r^2, count r < thr
  for (long long i = (long long)blockIdx.x * T + threadIdx.x; i < np; i += (long long)gridDim.x * T) {
    const double d = dp[i];
    acc[0] += d;
    acc[1] += d * d;
    acc[2] += d < threshold ? 1.0 : 0.0;
  }
  for (long long i = (long long)blockIdx.x * T + threadIdx.x; i < nr; i += (long long)gridDim.x * T) {
    const double d = dr[i];
    acc[3] += d;
    acc[4] += d * d;
    acc[5] += d < threshold ? 1.0 : 0.0;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double w = shine::wave_sum_d(acc[k]);
    if ((threadIdx.x & 63) == 0) sm.v[k][threadIdx.x >> 6] = w;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    double t = 0.0;
    for (int w = 0; w < T / 64; ++w) t += sm.v[threadIdx.x][w];
    part[6 * blockIdx.x + threadIdx.x] = t;
  }
  if (!shine::arrive_last(done, gridDim.x, &is_last)) return;  // (the entry point clears `done` in front of every launch)
  if (threadIdx.x < 6) {
    double t = 0.0;
    for (unsigned int b = 0; b < gridDim.x; ++b) t += part[6 * b + threadIdx.x];
    out[threadIdx.x] = t;
  }
  if (threadIdx.x == 6) out[6] = (double)np;
  if (threadIdx.x == 7) out[7] = (double)nr;
}

// the workspace of shine_eval_grid_count, read again by shine_eval_grid_emit
struct GridScratch {
  unsigned long long *k0, *k1, *v0, *v1;
  unsigned char *fflag, *cflag;
  int *frank, *crank;
  void* tmp;
  size_t tmp_bytes, bytes;
};

int grid_scratch(void* ws, long long n, hipStream_t st, GridScratch* s) {
  shine::Arena c(ws);
  s->k0 = c.take<unsigned long long>((size_t)n);
  s->k1 = c.take<unsigned long long>((size_t)n);
  s->v0 = c.take<unsigned long long>((size_t)n);
  s->v1 = c.take<unsigned long long>((size_t)n);
  s->fflag = c.take<unsigned char>((size_t)n);
  s->cflag = c.take<unsigned char>((size_t)n);
  s->frank = c.take<int>((size_t)n);
  s->crank = c.take<int>((size_t)n);
  size_t sort_bytes = 0, scan_bytes = 0;
  SHINE_HIP_CHECK(shine::prim_sort_pairs_u64(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, (size_t)n, 0u, 64u, st));
  SHINE_HIP_CHECK(shine::prim_scan_flags(nullptr, scan_bytes, nullptr, nullptr, (size_t)n, st));
  s->tmp_bytes = sort_bytes > scan_bytes ? sort_bytes : scan_bytes;
  s->tmp = c.take_bytes(s->tmp_bytes);
  s->bytes = c.bytes();
  return SHINE_OK;
}

// device-to-host: last rank + last flag = number of runs
int run_count(const int* rank, const unsigned char* flags, long long n, hipStream_t st, int64_t* out) {
  int r = 0;
  unsigned char f = 0;
  SHINE_HIP_CHECK(hipMemcpyAsync(&r, rank + n - 1, 4, hipMemcpyDeviceToHost, st));
  SHINE_HIP_CHECK(hipMemcpyAsync(&f, flags + n - 1, 1, hipMemcpyDeviceToHost, st));
  SHINE_HIP_CHECK(hipStreamSynchronize(st));
  *out = (int64_t)r + f;
  return SHINE_OK;
}

#define LAUNCH(kernel, count, ...)                                                            \
  do {                                                                                        \
    hipLaunchKernelGGL(kernel, dim3(grid_of(count)), dim3(T), 0, st, __VA_ARGS__);            \
    SHINE_HIP_CHECK(hipGetLastError());                                                       \
  } while (0)

// the front of both voxel down-samplers: keys, the stable sort of (key, index), run flags and run ranks
int voxel_runs(const GridScratch& s, const double* points, long long nn, const double* origin, double voxel, hipStream_t st) {
  const Vec3 o{origin[0], origin[1], origin[2]};
  LAUNCH(k_voxel_keys, nn, points, nn, o, voxel, s.k0, s.v0);
  size_t tb = s.tmp_bytes;
  SHINE_HIP_CHECK(shine::prim_sort_pairs_u64(s.tmp, tb, s.k0, s.k1, s.v0, s.v1, (size_t)nn, 0u, 63u, st));
  LAUNCH(k_run_flags, nn, (const unsigned long long*)s.k1, nn, 0, s.fflag);
  tb = s.tmp_bytes;
  SHINE_HIP_CHECK(shine::prim_scan_flags(s.tmp, tb, s.fflag, s.frank, (size_t)nn, st));
  return SHINE_OK;
}

}  // namespace

extern "C" int shine_eval_fine_per_coarse(void) { return FINE_PER_COARSE; }

extern "C" int shine_eval_bounds(const double* points, int64_t n, void* workspace, size_t* workspace_bytes, double* bounds_out,
                                 void* stream) {
  if (!workspace_bytes || bad_count(n)) return shine::set_error(SHINE_E_INVALID, "shine_eval_bounds: bad size (n must be < 2^31)");
  shine::Arena c(workspace);
  double* part = c.take<double>((size_t)RED_BLOCKS * 6);
  SHINE_WORKSPACE_GATE(c.bytes(), workspace, workspace_bytes, "shine_eval_bounds");
  if (n == 0 || !points || !bounds_out) return shine::set_error(SHINE_E_INVALID, "shine_eval_bounds: empty cloud or null argument");
  hipStream_t st = (hipStream_t)stream;
  const int blocks = (int)(grid_of(n) < (unsigned)RED_BLOCKS ? grid_of(n) : (unsigned)RED_BLOCKS);
  hipLaunchKernelGGL(k_bounds_partial, dim3(blocks), dim3(T), 0, st, points, (long long)n, part);
  SHINE_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_bounds_final, dim3(1), dim3(64), 0, st, (const double*)part, blocks, bounds_out);
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}

extern "C" int shine_eval_box_mask(const double* points, int64_t n, const double* min_bound, const double* max_bound,
                                   uint8_t* drop_out, void* stream) {
  if (bad_count(n) || !min_bound || !max_bound) return shine::set_error(SHINE_E_INVALID, "shine_eval_box_mask: bad size or null bound");
  if (n == 0) return SHINE_OK;
  if (!points || !drop_out) return shine::set_error(SHINE_E_INVALID, "shine_eval_box_mask: null argument");
  hipStream_t st = (hipStream_t)stream;
  const Vec3 lo{min_bound[0], min_bound[1], min_bound[2]}, hi{max_bound[0], max_bound[1], max_bound[2]};
  LAUNCH(k_outside_box, n, points, (long long)n, lo, hi, drop_out);
  return SHINE_OK;
}

extern "C" int shine_eval_sample_mesh(const double* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, int64_t n,
                                      uint64_t seed, const double* uniforms, void* workspace, size_t* workspace_bytes,
                                      double* points_out, int32_t* tri_out, void* stream) {
  if (!workspace_bytes || bad_count(n_verts) || bad_count(n_faces) || bad_count(n))
    return shine::set_error(SHINE_E_INVALID, "shine_eval_sample_mesh: bad sizes (V, F and n must be < 2^31)");
  const long long nf = n_faces;
  const int blocks = (int)((nf + 4 * T - 1) / (4 * T));
  shine::Arena c(workspace);
  double* cum = c.take<double>((size_t)nf);
  double* tot = c.take<double>((size_t)(blocks > 0 ? blocks : 1));
  SHINE_WORKSPACE_GATE(c.bytes(), workspace, workspace_bytes, "shine_eval_sample_mesh");
  if (n == 0) return SHINE_OK;
  if (nf == 0) return shine::set_error(SHINE_E_INVALID, "shine_eval_sample_mesh: a mesh without triangles cannot be sampled");
  if (!verts || !faces || !points_out) return shine::set_error(SHINE_E_INVALID, "shine_eval_sample_mesh: null argument");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_area_scan_block, dim3(blocks), dim3(T), 0, st, verts, faces, nf, (long long)n_verts, cum, tot);
  SHINE_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_area_scan_totals, dim3(1), dim3(64), 0, st, tot, blocks);
  SHINE_HIP_CHECK(hipGetLastError());
  LAUNCH(k_area_scan_add, nf, cum, (const double*)tot, nf);
  double total = 0.0;
  SHINE_HIP_CHECK(hipMemcpyAsync(&total, cum + nf - 1, 8, hipMemcpyDeviceToHost, st));
  SHINE_HIP_CHECK(hipStreamSynchronize(st));
  if (!(total > 0.0) || total == INFINITY)
    return shine::set_error(SHINE_E_INVALID, "shine_eval_sample_mesh: the mesh has no area (or a vertex is not finite)");
  LAUNCH(k_sample, n, verts, faces, nf, (const double*)cum, (long long)n, (unsigned long long)seed, uniforms, points_out, tri_out);
  return SHINE_OK;
}

extern "C" int shine_eval_voxel_down(const double* points, int64_t n, const double* origin, double voxel, void* workspace,
                                     size_t* workspace_bytes, double* points_out, uint64_t* keys_out, int64_t* n_out,
                                     void* stream) {
  if (!workspace_bytes || bad_count(n)) return shine::set_error(SHINE_E_INVALID, "shine_eval_voxel_down: bad size (n must be < 2^31)");
  hipStream_t st = (hipStream_t)stream;
  GridScratch s;
  if (int rc = grid_scratch(workspace, n, st, &s)) return rc;
  SHINE_WORKSPACE_GATE(s.bytes, workspace, workspace_bytes, "shine_eval_voxel_down");
  if (!n_out || !origin || !(voxel > 0.0)) return shine::set_error(SHINE_E_INVALID, "shine_eval_voxel_down: null argument or voxel <= 0");
  *n_out = 0;
  if (n == 0) return SHINE_OK;
  if (!points || !points_out) return shine::set_error(SHINE_E_INVALID, "shine_eval_voxel_down: null argument");
  const long long nn = n;
  if (int rc = voxel_runs(s, points, nn, origin, voxel, st)) return rc;
  // points_out has room for n rows (the caller cuts it to *n_out)
  LAUNCH(k_voxel_mean, nn, points, (const unsigned long long*)s.k1, (const unsigned long long*)s.v1,
         (const unsigned char*)s.fflag, (const int*)s.frank, nn, points_out, (unsigned long long*)keys_out);
  return run_count(s.frank, s.fflag, nn, st, n_out);
}

extern "C" int shine_voxel_down_attr(const double* points, const double* attrs, int32_t n_attr, int64_t n, const double* origin,
                                     double voxel, void* workspace, size_t* workspace_bytes, double* points_out,
                                     double* attrs_out, uint64_t* keys_out, int64_t* n_out, void* stream) {
  if (!workspace_bytes || bad_count(n)) return shine::set_error(SHINE_E_INVALID, "shine_voxel_down_attr: bad size (n must be < 2^31)");
  if (n_attr < 1 || n_attr > MAX_ATTR) return shine::set_error(SHINE_E_INVALID, "shine_voxel_down_attr: n_attr must be 1..4");
  // (the checks that are host arithmetic come first: the scratch size below is rocPRIM's answer for the current device)
  if (workspace && (!n_out || !origin || !(voxel > 0.0)))
    return shine::set_error(SHINE_E_INVALID, "shine_voxel_down_attr: null argument or voxel <= 0");
  if (workspace && n > 0 && (!points || !attrs || !points_out || !attrs_out))
    return shine::set_error(SHINE_E_INVALID, "shine_voxel_down_attr: null argument");
  hipStream_t st = (hipStream_t)stream;
  GridScratch s;
  if (int rc = grid_scratch(workspace, n, st, &s)) return rc;
  SHINE_WORKSPACE_GATE(s.bytes, workspace, workspace_bytes, "shine_voxel_down_attr");
  *n_out = 0;
  if (n == 0) return SHINE_OK;
  const long long nn = n;
  if (int rc = voxel_runs(s, points, nn, origin, voxel, st)) return rc;  // (shine_eval_voxel_down's keys, in its order)
  LAUNCH(k_voxel_mean_attr, nn, points, attrs, (int)n_attr, (const unsigned long long*)s.k1, (const unsigned long long*)s.v1,
         (const unsigned char*)s.fflag, (const int*)s.frank, nn, points_out, attrs_out, (unsigned long long*)keys_out);
  return run_count(s.frank, s.fflag, nn, st, n_out);
}

extern "C" int shine_eval_grid_count(const double* ref, int64_t n, const double* origin, double cell, void* workspace,
                                     size_t* workspace_bytes, int64_t* counts_out, void* stream) {
  if (!workspace_bytes || bad_count(n) || n == 0)
    return shine::set_error(SHINE_E_INVALID, "shine_eval_grid_count: bad size (0 < n < 2^31)");
  hipStream_t st = (hipStream_t)stream;
  GridScratch s;
  if (int rc = grid_scratch(workspace, n, st, &s)) return rc;
  SHINE_WORKSPACE_GATE(s.bytes, workspace, workspace_bytes, "shine_eval_grid_count");
  if (!ref || !origin || !counts_out || !(cell > 0.0)) return shine::set_error(SHINE_E_INVALID, "shine_eval_grid_count: null argument or cell <= 0");
  const Vec3 o{origin[0], origin[1], origin[2]};
  const long long nn = n;
  LAUNCH(k_grid_keys, nn, ref, nn, o, cell, s.k0, s.v0);
  size_t tb = s.tmp_bytes;
  SHINE_HIP_CHECK(shine::prim_sort_pairs_u64(s.tmp, tb, s.k0, s.k1, s.v0, s.v1, (size_t)nn, 0u, 63u, st));
  LAUNCH(k_run_flags, nn, (const unsigned long long*)s.k1, nn, 0, s.fflag);
  LAUNCH(k_run_flags, nn, (const unsigned long long*)s.k1, nn, LOCAL_BITS, s.cflag);
  tb = s.tmp_bytes;
  SHINE_HIP_CHECK(shine::prim_scan_flags(s.tmp, tb, s.fflag, s.frank, (size_t)nn, st));
  tb = s.tmp_bytes;
  SHINE_HIP_CHECK(shine::prim_scan_flags(s.tmp, tb, s.cflag, s.crank, (size_t)nn, st));
  if (int rc = run_count(s.frank, s.fflag, nn, st, counts_out)) return rc;
  return run_count(s.crank, s.cflag, nn, st, counts_out + 1);
}

extern "C" int shine_eval_grid_emit(const double* ref, int64_t n, const void* workspace, size_t workspace_bytes, int64_t n_fine,
                                    int64_t n_coarse, void* grid, size_t* grid_bytes, void* stream) {
  if (!grid_bytes || bad_count(n) || n == 0 || n_fine < 1 || n_fine > n || n_coarse < 1 || n_coarse > n_fine)
    return shine::set_error(SHINE_E_INVALID, "shine_eval_grid_emit: bad sizes");
  const GridLayout L = grid_layout(grid, n, n_fine, n_coarse);
  if (!grid) {  // (by hand, not SHINE_WORKSPACE_GATE: the grid is a result the caller keeps, and its message says so)
    *grid_bytes = L.bytes;
    return SHINE_OK;
  }
  if (*grid_bytes < L.bytes) return shine::set_error(SHINE_E_INVALID, "shine_eval_grid_emit: grid buffer too small");
  hipStream_t st = (hipStream_t)stream;
  GridScratch s;
  if (int rc = grid_scratch(const_cast<void*>(workspace), n, st, &s)) return rc;
  SHINE_WORKSPACE_FITS(s.bytes, workspace, workspace_bytes, "shine_eval_grid_emit");  // (the one shine_eval_grid_count filled)
  if (!ref) return shine::set_error(SHINE_E_INVALID, "shine_eval_grid_emit: null ref");
  const long long nn = n;
  SHINE_HIP_CHECK(hipMemsetAsync(L.table, 0xff, (size_t)L.cap * sizeof(Cell), st));
  LAUNCH(k_grid_emit, nn, ref, (const unsigned long long*)s.k1, (const unsigned long long*)s.v1, (const unsigned char*)s.fflag,
         (const unsigned char*)s.cflag, (const int*)s.frank, (const int*)s.crank, nn, L.pts, L.sidx, L.fine, L.coarse);
  const unsigned int bits = log2_of(L.cap);
  LAUNCH(k_coarse_insert, n_coarse, (const Cell*)L.coarse, (long long)n_coarse, L.table, 64u - bits, (unsigned int)(L.cap - 1));
  return SHINE_OK;
}

extern "C" int shine_eval_nn_search(const void* grid, int64_t n_ref, int64_t n_fine, int64_t n_coarse, const double* origin,
                                    double cell, const int64_t* cells_per_axis, const double* query, int64_t n_query,
                                    double truncation, void* workspace, size_t* workspace_bytes, int32_t* index_out,
                                    double* dist_out, uint8_t* keep_out, int32_t* stats_out, void* stream) {
  if (!workspace_bytes || bad_count(n_ref) || n_ref == 0 || bad_count(n_query) || n_fine < 1 || n_fine > n_ref || n_coarse < 1 ||
      n_coarse > n_fine)
    return shine::set_error(SHINE_E_INVALID, "shine_eval_nn_search: bad sizes");
  hipStream_t st = (hipStream_t)stream;
  const long long nq = n_query;
  shine::Arena c(workspace);
  auto* k0 = c.take<unsigned long long>((size_t)nq);
  auto* k1 = c.take<unsigned long long>((size_t)nq);
  auto* v0 = c.take<unsigned long long>((size_t)nq);
  auto* v1 = c.take<unsigned long long>((size_t)nq);
  size_t sort_bytes = 0;
  SHINE_HIP_CHECK(shine::prim_sort_pairs_u64(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, (size_t)nq, 0u, 64u, st));
  void* tmp = c.take_bytes(sort_bytes);
  SHINE_WORKSPACE_GATE(c.bytes(), workspace, workspace_bytes, "shine_eval_nn_search");
  if (nq == 0) return SHINE_OK;
  if (!grid || !origin || !cells_per_axis || !query || !index_out || !dist_out || !keep_out || !(cell > 0.0) || !(truncation >= 0.0))
    return shine::set_error(SHINE_E_INVALID, "shine_eval_nn_search: null argument, cell <= 0 or truncation < 0");
  GridDev g;
  if (!grid_dev(grid, n_ref, n_fine, n_coarse, origin, cell, cells_per_axis, &g))
    return shine::set_error(SHINE_E_INVALID, "shine_eval_nn_search: cells_per_axis out of range (1 .. 2^21)");
  LAUNCH(k_query_keys, nq, query, nq, g.o, cell, k0, v0);
  SHINE_HIP_CHECK(shine::prim_sort_pairs_u64(tmp, sort_bytes, k0, k1, v0, v1, (size_t)nq, 0u, 63u, st));
  if (stats_out) SHINE_HIP_CHECK(hipMemsetAsync(stats_out, 0, 8, st));
  LAUNCH(k_nn_search, nq, g, query, (const unsigned long long*)v1, nq, truncation, index_out, dist_out, keep_out, stats_out);
  return SHINE_OK;
}

extern "C" int shine_eval_metrics(const double* dist_p, int64_t n_p, const double* dist_r, int64_t n_r, double threshold,
                                  void* workspace, size_t* workspace_bytes, double* sums_out, void* stream) {
  if (!workspace_bytes || bad_count(n_p) || bad_count(n_r)) return shine::set_error(SHINE_E_INVALID, "shine_eval_metrics: bad sizes");
  shine::Arena c(workspace);
  double* part = c.take<double>((size_t)RED_BLOCKS * 6);
  unsigned int* done = c.take<unsigned int>(1);
  SHINE_WORKSPACE_GATE(c.bytes(), workspace, workspace_bytes, "shine_eval_metrics");
  if (!sums_out || (n_p && !dist_p) || (n_r && !dist_r)) return shine::set_error(SHINE_E_INVALID, "shine_eval_metrics: null argument");
  hipStream_t st = (hipStream_t)stream;
  const long long big = n_p > n_r ? n_p : n_r;
  unsigned blocks = grid_of(big);
  blocks = blocks < 1 ? 1 : (blocks > (unsigned)RED_BLOCKS ? (unsigned)RED_BLOCKS : blocks);
  SHINE_HIP_CHECK(hipMemsetAsync(done, 0, 4, st));
  hipLaunchKernelGGL(k_metrics, dim3(blocks), dim3(T), 0, st, dist_p, (long long)n_p, dist_r, (long long)n_r, threshold, part, done,
                     sums_out);
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}
