// shine_term_dev.hpp — the device side every lane-per-row training step shares (k_sem_step, k_normal_step / k_consistency_step,
// k_time_step / k_ray_step; the scatter also serves k_interp_bwd, the grid sum k_sem_bwd; DESIGN.md 3.21, "the device contract of
// a term step"): the launch shape, the transposed feature-grad scatter, the workgroup's partial and the two-level ticket sum over
// the grid.  A step supplies its gather and chain, the eight per-corner coefficients of its scatter, the layout of its partial
// vector and the sinks of the grid sum.  Every piece is __forceinline__, and a kernel takes a piece only where it costs it no
// spilled SGPR, no LDS, no scratch and no wave per SIMD against its own lines (profiles/term_tail_refactor_resources.txt): the
// gterm body keeps its scatter and its partial, the point-step body its partial and its grid sum, each with a note of the number.
#pragma once
#include "shine_arrive.hpp"
#include "shine_internal.hpp"

namespace shine {

// ---- launch shape: four waves per workgroup, a tile of 64 lanes each, at most kMaxBlocks workgroups with a grid stride beyond
//      (64 K lanes); it depends on the tile count alone, so equal batches sum in equal order.  (One wave per workgroup was
//      measured on the semantic step at N = 4096: 8 us less with the head frozen, 13 us MORE with it training, where 64 partial
//      vectors instead of 16 meet in the ticket sums; not kept.  DESIGN.md 3.15.)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;  // waves of a workgroup, a tile each
constexpr int kMaxBlocks = 256;
constexpr int kGroup = 16;  // workgroups per first-level run
constexpr int kGroups = kMaxBlocks / kGroup;
constexpr size_t kCounterBytes = 256;  // [0] run-level ticket, [1..kGroups] first-level tickets
static_assert((kGroups + 1) * sizeof(unsigned) <= kCounterBytes, "counters");

inline unsigned term_blocks(long long tiles) {
  const long long b = (tiles + kWaves - 1) / kWaves;
  return (unsigned)(b > kMaxBlocks ? kMaxBlocks : b);
}

// a ROLLED loop over weight rows (scalar loads), n trips per iteration
#define TERM_LOOP_STR(x) #x
#define TERM_ROW_LOOP(n) _Pragma(TERM_LOOP_STR(clang loop vectorize(disable) interleave(disable) unroll_count(n)))

// (The level gathers are not here.  The `+= w * r` form of k_sem_step / k_sem_query / k_query_points and the fmaf form of the
// gterm and point-step bodies round differently, and either one behind a helper cost its kernels registers: the `+=` form one more
// spilled SGPR in k_sem_query<3, *> and k_sem_step<2, true> and 12 more in k_query_points<4, *>, the fmaf form 12 to 24 VGPRs in
// every build with A = df/dx.  profiles/term_tail_refactor_resources.txt.)

// ---- the feature-grad scatter with the lanes TRANSPOSED: one atomic instruction covers 8 rows x the 8 features of one corner row
//      each (8 x 32 contiguous bytes) instead of 64 different rows x 4 bytes — an eighth of the memory-side transactions.
// The per-row vector v (d loss / d feature up to the corner coefficient) through the wave's LDS rows once: [row][feature] in,
// gval[G] = v[row G * 8 + (lane >> 3)][lane & 7] out.  st: the wave's staging rows (>= 64 * F floats, free at this point).
__device__ __forceinline__ void stage_row_grads(float* st, int lane, const float (&v)[F], float (&gval)[8]) {
#pragma unroll
  for (int q = 0; q < F; ++q) st[lane * F + q] = v[q];
  wave_lds_fence();
#pragma unroll
  for (int G = 0; G < 8; ++G) gval[G] = st[G * 64 + lane];
  wave_lds_fence();
}

// One level's rows += cf[c] * v for the eight corners of every lane's point: the corner ids and coefficients of the source row
// come by shuffle from lane G * 8 + sub.  hit: the lane has a point with corners at this level; miss: it has a point without —
// all eight corners address the trash row, which receives sum_c cf[c] * v, one atomic per wave and feature instead of 64 per
// missing point on the same 32 bytes (same-address atomics serialise at the memory controller).  Called by the whole wave.
__device__ __forceinline__ void scatter_corner_rows(const LevelDev& Lv, const int (&ids)[8], bool hit, bool miss,
                                                    const float (&cf)[8], const float (&v)[F], const float (&gval)[8], int lane) {
  const int sub = lane >> 3, fi = lane & 7;
  float csum = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    csum += cf[c];
    const int sid = hit ? ids[c] : -1;
#pragma unroll
    for (int G = 0; G < 8; ++G) {
      const int id = __shfl(sid, G * 8 + sub, 64);
      const float cv = __shfl(cf[c], G * 8 + sub, 64);
      if (id >= 0) atomic_add_f32(Lv.grad + (long long)id * F + fi, cv * gval[G]);
    }
  }
  if (__any(miss)) {
    const float cm = miss ? csum : 0.f;
#pragma unroll
    for (int q = 0; q < F; ++q) {
      const float tsum = wave_sum(cm * v[q]);
      if (lane == 0 && tsum != 0.f) atomic_add_f32(Lv.grad + Lv.rows * F + q, tsum);
    }
  }
}

// ---- the workgroup's partial: every wave stages its NV accumulators (s_stage: NV * kThreads floats, free after a barrier
//      behind the tile loop), wave 0 adds waves 1..kWaves-1 to its own in index order.  Called by every thread of the workgroup
//      in block-uniform control flow; afterwards wave 0 maps vals into the step's partial layout.
template <int NV>
__device__ __forceinline__ void tile_partial(float (&vals)[NV], float* s_stage, int wv, int lane) {
#pragma unroll
  for (int v = 0; v < NV; ++v) s_stage[(wv * NV + v) * 64 + lane] = vals[v];
  __syncthreads();
  if (wv == 0) {
#pragma unroll
    for (int ww = 1; ww < kWaves; ++ww) {
#pragma unroll
      for (int v = 0; v < NV; ++v) vals[v] += s_stage[(ww * NV + v) * 64 + lane];
    }
  }
}

// ---- the sum over the grid of the workgroups' partials, in two ticket levels (shine_arrive.hpp): the last workgroup of each run
//      of kGroup to arrive sums that run's partials in index order, the last run to finish sums the run sums in index order and
//      hands every sum to the caller.  Fixed order throughout: the results are bit-identical from call to call.
struct GridSumWs {
  unsigned* cnt;        // [1 + kGroups] tickets: [0] run level, [1..] first level; zero before the launch, zero after it
  float *part, *run;    // [kMaxBlocks][STRIDE] partials (stored by their workgroups before the call), [kGroups][STRIDE] run sums
  double *lpart, *lrun; // [kMaxBlocks][NL], [kGroups][NL] fp64 loss partials and run sums (NL = 0: unused)
};
// One level of the fp64 loss sums, by the 64 lanes of one wave: a lane per partial and sum (per-lane addresses; the partial is
// cleared behind the read), then a fixed-order sum over the lanes.  -> lane q < NL holds sum q of src[first .. first + count).
template <unsigned NL>
__device__ __forceinline__ double loss_lanes_sum(double* src, unsigned first, unsigned count, unsigned slots) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned li = lane / NL, lc = lane % NL;  // (partial, which of its sums)
  const double v = li < count ? src[(size_t)(first + li) * NL + lc] : 0.0;
  if (li < count) src[(size_t)(first + li) * NL + lc] = 0.0;
  double s = 0.0;
  for (unsigned b = 0; b < slots; ++b) s += __shfl(v, (int)(NL * b + lc), 64);
  return s;
}

// The floats are walked in columns of four: all of them with `full`, else those from column C0 on (C0 = STRIDE / 4: none — a
// frozen decoder; the semantic head keeps its loss's column).  CLEAR: whoever sums a partial clears it behind itself, so the whole
// workspace is zero again when the launch ends.  The finishing workgroup calls sink(k, float4 of sums k .. k + 3) for every column
// it summed and, with NL > 0, fin(sums) from one lane.  Called by every thread of every workgroup; -> whether this workgroup
// finished the sum (block-uniform).  verdict: one LDS word.  (The guard in front of each walk keeps a frozen decoder's launch
// at one live flag instead of a first column carried across the tile loop: two spilled SGPRs.)
template <int STRIDE, int C0, bool CLEAR, int NL, class Sink, class Fin>
__device__ __forceinline__ bool grid_sum_two_level(const GridSumWs& w, bool full, unsigned* verdict, Sink sink, Fin fin) {
  static_assert(STRIDE % 4 == 0, "float4 walk");
  static_assert(kGroup * NL <= 64 && kGroups * NL <= 64, "a run's loss partials are read by one wave, a lane each");
  const unsigned G = gridDim.x;
  const unsigned grp = blockIdx.x / kGroup;
  const unsigned g0 = grp * kGroup;
  const unsigned gsz = (G - g0) < (unsigned)kGroup ? (G - g0) : (unsigned)kGroup;
  const unsigned ngrp = (G + kGroup - 1) / kGroup;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

  if (!arrive_last(w.cnt + 1 + grp, gsz, verdict)) return false;
  if (full || C0 < STRIDE / 4) {
    for (int c = (full ? 0 : C0) + threadIdx.x; c < STRIDE / 4; c += kThreads) {
      float4 s = zero4;
      for (unsigned b = 0; b < gsz; ++b) {
        float4* src = reinterpret_cast<float4*>(w.part + (size_t)(g0 + b) * STRIDE + 4 * c);
        const float4 v = *src;
        s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
        if constexpr (CLEAR) *src = zero4;  // (read once, by this thread)
      }
      *reinterpret_cast<float4*>(w.run + (size_t)grp * STRIDE + 4 * c) = s;
    }
  }
  if constexpr (NL > 0) {
    if (threadIdx.x < 64) {
      const double s = loss_lanes_sum<NL>(w.lpart, g0, gsz, kGroup);
      if (threadIdx.x < NL) w.lrun[(size_t)grp * NL + threadIdx.x] = s;
    }
  }
  if (threadIdx.x == 0) __hip_atomic_store(w.cnt + 1 + grp, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // for the next call

  if (!arrive_last(w.cnt, ngrp, verdict)) return false;
  if (full || C0 < STRIDE / 4) {
    for (int c = (full ? 0 : C0) + threadIdx.x; c < STRIDE / 4; c += kThreads) {
      float4 s = zero4;
      for (unsigned r = 0; r < ngrp; ++r) {
        float4* src = reinterpret_cast<float4*>(w.run + (size_t)r * STRIDE + 4 * c);
        const float4 v = *src;
        s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
        if constexpr (CLEAR) *src = zero4;
      }
      sink(4 * c, s);
    }
  }
  if constexpr (NL > 0) {
    if (threadIdx.x < 64) {
      const double s = loss_lanes_sum<NL>(w.lrun, 0u, ngrp, kGroups);
      double sums[NL];
#pragma unroll
      for (int q = 0; q < NL; ++q) sums[q] = NL == 1 ? s : __shfl(s, q, 64);  // (read by lane 0; one sum: it holds it)
      if (threadIdx.x == 0) fin(sums);
    }
  }
  if (threadIdx.x == 0) __hip_atomic_store(w.cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

}  // namespace shine
