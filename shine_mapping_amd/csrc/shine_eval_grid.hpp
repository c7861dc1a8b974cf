// shine_eval_grid.hpp — the two-level search grid of shine_eval.hip (built by shine_eval_grid_count / shine_eval_grid_emit), as
// the kernels that walk it see it: shine_eval.hip's nearest-neighbour search and shine_frame_nn.hip's k-nearest-neighbour
// search.  Layout and rules are those of shine_eval.hip's header comment and DESIGN.md §3.10.
#pragma once
#include "shine_internal.hpp"

namespace shine {
namespace grid {

constexpr int FINE_BITS = 2;                     // fine cells per coarse cell edge = 1 << FINE_BITS
constexpr int FINE_PER_COARSE = 1 << FINE_BITS;
constexpr int LOCAL_BITS = 3 * FINE_BITS;        // low bits of a sort key: the fine cell inside its coarse cell
constexpr int AXIS_BITS = 21;                    // fine cell index bits per axis
constexpr int COARSE_BITS = AXIS_BITS - FINE_BITS;
constexpr long long AXIS_MAX = (1ll << AXIS_BITS) - 1;
constexpr double MARGIN = 1.0 / (1 << 20);       // cell units: slack of every box bound (cell assignment rounds at ~2^-32)
constexpr unsigned long long EMPTY = ~0ull;

inline bool bad_count(int64_t n) { return n < 0 || n >= (1ll << 31); }

struct Vec3 {
  double x, y, z;
};

struct Cell {  // a fine-cell entry, or a slot of the coarse table
  unsigned long long key;
  int first, end;
};

// sort key of a fine cell (ix, iy, iz): the coarse cell (ix >> 2, ...) in bits 6.., the fine cell inside it in bits 0..5
__device__ __forceinline__ unsigned long long grid_key(unsigned long long ix, unsigned long long iy, unsigned long long iz) {
  const unsigned long long m = FINE_PER_COARSE - 1;
  const unsigned long long local = ((ix & m) << (2 * FINE_BITS)) | ((iy & m) << FINE_BITS) | (iz & m);
  return (((ix >> FINE_BITS) << (2 * COARSE_BITS)) | ((iy >> FINE_BITS) << COARSE_BITS) | (iz >> FINE_BITS)) << LOCAL_BITS | local;
}

__device__ __forceinline__ unsigned long long coarse_key(long long cx, long long cy, long long cz) {
  return ((unsigned long long)cx << (2 * COARSE_BITS)) | ((unsigned long long)cy << COARSE_BITS) | (unsigned long long)cz;
}

__device__ __forceinline__ unsigned int coarse_slot(unsigned long long key, unsigned int shift) {
  return (unsigned int)((key * 0x9E3779B97F4A7C15ull) >> shift);
}

// distance from t (cell units) to the box [lo, lo + w] widened by MARGIN, along one axis
__device__ __forceinline__ double axis_gap(double t, double lo, double w) {
  const double below = (lo - MARGIN) - t, above = t - (lo + w + MARGIN);
  const double g = fmax(fmax(below, above), 0.0);
  return g;
}

struct GridDev {
  const double* pts;   // [n][3] reference points, sorted by cell
  const int* sidx;     // [n] their indices in the caller's array
  const Cell* fine;    // [n_fine]
  const Cell* table;   // [mask + 1] coarse cells, open addressing
  unsigned int shift, mask;
  Vec3 o;
  double cell;
  long long cmax[3];   // largest coarse cell index per axis
};

// the fine / end range of the occupied coarse cell `ck` (f0 == f1: the cell is empty)
__device__ __forceinline__ void coarse_probe(const GridDev& g, unsigned long long ck, int& f0, int& f1) {
  unsigned int slot = coarse_slot(ck, g.shift);
  f0 = 0;
  f1 = 0;
  for (unsigned int tries = 0; tries <= g.mask; ++tries) {
    const Cell e = g.table[slot];
    if (e.key == ck) {
      f0 = e.first;
      f1 = e.end;
      return;
    }
    if (e.key == EMPTY) return;
    slot = (slot + 1) & g.mask;
  }
}

struct GridLayout {
  double* pts;
  int* sidx;
  Cell* fine;
  Cell* coarse;
  Cell* table;
  long long cap;
  size_t bytes;
};

inline GridLayout grid_layout(void* buf, long long n, long long n_fine, long long n_coarse) {
  Arena c(buf);
  GridLayout L;
  L.pts = c.take<double>((size_t)n * 3);
  L.sidx = c.take<int>((size_t)n);
  L.fine = c.take<Cell>((size_t)n_fine);
  L.coarse = c.take<Cell>((size_t)n_coarse);
  long long cap = 16;
  while (cap < 2 * n_coarse) cap <<= 1;
  L.cap = cap;
  L.table = c.take<Cell>((size_t)cap);
  L.bytes = c.bytes();
  return L;
}

inline unsigned int log2_of(long long pow2) {
  unsigned int b = 0;
  while ((1ll << b) < pow2) ++b;
  return b;
}

// the kernel-side view of a grid buffer written by shine_eval_grid_emit; false: cells_per_axis out of range (1 .. 2^21)
inline bool grid_dev(const void* grid, long long n_ref, long long n_fine, long long n_coarse, const double* origin, double cell,
                     const int64_t* cells_per_axis, GridDev* g) {
  const GridLayout L = grid_layout(const_cast<void*>(grid), n_ref, n_fine, n_coarse);
  g->pts = L.pts;
  g->sidx = L.sidx;
  g->fine = L.fine;
  g->table = L.table;
  g->mask = (unsigned int)(L.cap - 1);
  g->shift = 64u - log2_of(L.cap);
  g->o = Vec3{origin[0], origin[1], origin[2]};
  g->cell = cell;
  for (int a = 0; a < 3; ++a) {
    if (cells_per_axis[a] < 1 || cells_per_axis[a] > AXIS_MAX + 1) return false;
    g->cmax[a] = (cells_per_axis[a] - 1) >> FINE_BITS;
  }
  return true;
}

}  // namespace grid
}  // namespace shine
