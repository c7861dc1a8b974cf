// shine_point_step_body.hpp — the lane-per-point step of a ONE-output head, shared by k_time_step (shine_time_step.hip) and
// k_ray_step (shine_ray_step.hip); DESIGN.md 3.22, 3.23:
//
//   f      = query_feature(x)                              levels summed, a miss contributes nothing; set_zero: the trash rows of
//                                                          the feature tables are re-zeroed by the launch
//   pred   = w3 . relu(W2 relu(W1f f + b1 [+ w_t ts]) + b2) + b3            W1 read in place with the policy's row stride
//   delta  = d (main loss) / d pred                        THE POLICY'S: BCE of a point, or the render of the point's ray
//   eik    = mean over weight > 0 of (1 - |g|)^2,  g = sigma d pred / d x  (EIK builds; 0 without a surface row)
//   grads += d loss / d {feature tables, W1, b1, W2, b2, w3, b3}
//
// One wave = one tile of batch rows at a time, lane = row (a term step's launch shape, shine_term_dev.hpp).  The head has ONE
// output, so its first-order backward is delta times the Jacobian chain the eikonal term needs anyway:
//   v2 = m2 .* w3,  v1 = m1 .* (W2^T v2),  J = W1f^T v1 = d pred / d f;   d2 = delta v2,  d1 = delta v1,  d f = delta J
// and with the eikonal term's second-order pieces (q = d loss / d g; r = sigma A q, a1 = m1 .* (W1f r), a2 = m2 .* (W2 a1),
// shine_gterm_body.hpp's chain with delta = 0) every weight gradient is ONE contraction over the tile's 64 staged rows:
//   dW1f += v1 (x) (delta f + r)     dW1[:,8] += v1 . (delta ts)     db1 += v1 . delta
//   dW2  += v2 (x) (delta h1 + a1)   db2 += v2 . delta               dw3 += delta h2 + a2      db3 += delta
// (the second-order part reaches W1f, W2 and w3 only: J depends on w_t, ts and the biases through the ReLU masks alone).
// Feature rows receive (w_c delta + sigma dw_c/dx . q) J through the shared transposed scatter.  The decoder layers are rolled
// loops over weight rows with scalar loads (3.18).
//
// The six weight grads and the P::NL loss sums (fp64 from the lanes up: [0] the main loss, [1] the eikonal term over the surface
// rows, the rest the policy's) are added in a fixed order inside a wave and a workgroup and in two ticket levels across
// workgroups (shine_arrive.hpp), so they are bit-identical from call to call; the workgroup that finishes the sum ADDS the grads,
// hands the sums to P::finish and leaves the workspace all zero.
//
// Of the shared tail (shine_term_dev.hpp) this body takes the launch shape and the scatter.  It keeps its own lines for the level
// gather (a helper: 12 to 24 more VGPRs in every EIK build) and for the workgroup's partial and the grid sum (through
// grid_sum_two_level k_ray_step<1, *, false> spills 8 more SGPRs and every k_ray_step<*, *, false> has 2 more DS reads; with the
// grid sum alone on its own lines k_time_step<1, true, true> and two more builds spill 2 more).
//
// A policy P has
//   Args                      the kernel's argument: PointStepArgs + what P reads
//   W1S, SHIFT                W1's row stride and whether its column F is a per-point shift of the first bias (ts)
//   NL                        loss sums (2 or 3)
//   Lane                      a lane's own values of the current tile
//   tiles(a), locate(a, t, lane, r, j, ln)   tile count; batch position r and source row j of (tile, lane), false: no row
//   load(a, j, ln), shift(ln)
//   delta(a, ln, valid, lane, y, st, acc)    -> d main / d pred; called by every lane of the wave, may use st[lane][32..64) and
//                                               fences before it returns if it did; adds to acc[0] (and its own sums)
//   store(a, r, y, delta)     the optional per-row outputs
//   grad_dst(a, k)            where entry k of the partial layout is added (null: nowhere)
//   finish(a, sums, ns)       one lane, with the grid's sums: writes the loss
#pragma once
#include "shine_term_dev.hpp"
#include "shine_term_host.hpp"

namespace shine {
namespace pstep {

// a lane's staging row (floats): [0,32) left operand | [32,64) right operand ([40] delta ts, [41] delta beside the 8-wide one)
// | [64] delta | [65,97) h2, then delta h2 + a2
constexpr int TST = 97;  // (odd: conflict-free column reads)
constexpr int R_TS = 40, R_D1 = 41, R_D2 = 64, R_H2 = 65;
// partial layout (floats): W1f [32][8] | w_t [32] | b1 [32] | W2 [32][32] | b2 [32] | w3 [32] | b3 [1] + 3 unused
constexpr int P_W1 = 0, P_WT = P_W1 + H * F, P_B1 = P_WT + H, P_W2 = P_B1 + H, P_B2 = P_W2 + H * H, P_W3 = P_B2 + H,
              P_B3 = P_W3 + H, PW = P_B3 + 4;
static_assert(PW % 4 == 0, "layout");

struct PointStepArgs {
  LevelSet ls;
  const float* coord;   // rows of `cstride` floats, x y z first
  const int* idx;       // [n] gather or null
  const float* weight;  // rows of `wstride` floats (EIK builds)
  const long long* n_surf;
  long long n;
  int cstride, wstride;
  int n_parts;  // entries of n_surf to add up (>= 1)
  float sigma, weight_e;
  const float* mlp[6];
  float* gW1;
  float* gW2;
  float* gw3;
  float* gb1;
  float* gb2;
  float* gb3;
  int want_wgrad;
  float* pred;  // at the batch position, or null
  float* loss_out;
  // the workspace's arrays: tickets ([0] run level, [1..kGroups] first level) | part [kMaxBlocks][PW] | run [kGroups][PW] |
  // loss_part [kMaxBlocks][NL] | loss_run [kGroups][NL]
  unsigned* cnt;
  float* part;
  float* run;
  double* lpart;
  double* lrun;
};

struct PointWork {
  unsigned* cnt;
  float *part, *run;
  double *lpart, *lrun;
  size_t bytes;
};
inline PointWork point_layout(void* workspace, int nl) {
  Arena ar(workspace);
  PointWork w;
  w.cnt = ar.take<unsigned>(kCounterBytes / sizeof(unsigned));
  w.part = ar.take<float>((size_t)kMaxBlocks * PW);
  w.run = ar.take<float>((size_t)kGroups * PW);
  w.lpart = ar.take<double>((size_t)kMaxBlocks * nl);
  w.lrun = ar.take<double>((size_t)kGroups * nl);
  w.bytes = ar.bytes();
  return w;
}

// The sum over the grid of the workgroups' partials, grid_sum_two_level's two ticket levels on this body's own lines (see the
// head of the file) with six tensors and NL loss sums: the
// last workgroup of each run of kGroup to arrive sums that run in index order, the last run to finish sums the run sums in
// index order, ADDS them to the six tensors and writes the loss.  Whoever sums a partial clears it behind itself and the tickets
// are reset, so the whole workspace is zero again when the launch ends.
template <class P>
__device__ __forceinline__ void point_grid_sum(const typename P::Args& a, bool wgrad, long long ns, unsigned* verdict) {
  constexpr unsigned NL = P::NL;
  static_assert(kGroup * NL <= 64 && kGroups * NL <= 64, "a run's loss partials are read by one wave, a lane each");
  const unsigned G = gridDim.x;
  const unsigned grp = blockIdx.x / kGroup;
  const unsigned g0 = grp * kGroup;
  const unsigned gsz = (G - g0) < (unsigned)kGroup ? (G - g0) : (unsigned)kGroup;
  const unsigned ngrp = (G + kGroup - 1) / kGroup;
  const unsigned lane = threadIdx.x & 63u;
  const unsigned li = lane / NL, lc = lane % NL;  // (partial, which of its sums)

  if (!arrive_last(a.cnt + 1 + grp, gsz, verdict)) return;
  if (wgrad) {
    for (int c = threadIdx.x; c < PW / 4; c += kThreads) {
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
      for (unsigned b = 0; b < gsz; ++b) {
        float4* src = reinterpret_cast<float4*>(a.part + (size_t)(g0 + b) * PW + 4 * c);
        const float4 v = *src;
        s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
        *src = make_float4(0.f, 0.f, 0.f, 0.f);  // (read once, by this thread: the workspace is left ALL zero)
      }
      *reinterpret_cast<float4*>(a.run + (size_t)grp * PW + 4 * c) = s;
    }
  }
  if (threadIdx.x < 64) {  // (a lane per partial and sum: per-lane addresses, then a fixed-order sum over the lanes)
    const double v = li < gsz ? a.lpart[(size_t)(g0 + li) * NL + lc] : 0.0;
    if (li < gsz) a.lpart[(size_t)(g0 + li) * NL + lc] = 0.0;
    double s = 0.0;
    for (unsigned b = 0; b < (unsigned)kGroup; ++b) s += __shfl(v, (int)(NL * b + lc), 64);
    if (lane < NL) a.lrun[(size_t)grp * NL + lc] = s;
  }
  if (threadIdx.x == 0) __hip_atomic_store(a.cnt + 1 + grp, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // for the next call

  if (!arrive_last(a.cnt, ngrp, verdict)) return;
  if (wgrad) {
    for (int k = threadIdx.x; k <= P_B3; k += kThreads) {
      float s = 0.f;
      for (unsigned r = 0; r < ngrp; ++r) s += a.run[(size_t)r * PW + k];
      float* dst = P::grad_dst(a, k);
      if (dst) dst[0] += s;
    }
    __syncthreads();  // (every read of the run sums is done before they are cleared)
    for (int c = threadIdx.x; c < PW / 4; c += kThreads)
      for (unsigned r = 0; r < ngrp; ++r) *reinterpret_cast<float4*>(a.run + (size_t)r * PW + 4 * c) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (threadIdx.x < 64) {
    const double v = li < ngrp ? a.lrun[(size_t)li * NL + lc] : 0.0;
    if (li < ngrp) a.lrun[(size_t)li * NL + lc] = 0.0;
    double s = 0.0;
    for (unsigned r = 0; r < (unsigned)kGroups; ++r) s += __shfl(v, (int)(NL * r + lc), 64);
    double sums[NL];  // (lane q holds sum q)
#pragma unroll
    for (unsigned q = 0; q < NL; ++q) sums[q] = __shfl(s, (int)q, 64);
    if (lane == 0) P::finish(a, sums, ns);
  }
  if (threadIdx.x == 0) __hip_atomic_store(a.cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int L, bool POLY, bool EIK, class P>
__device__ __forceinline__ void point_step_body(const typename P::Args& a, float* s_stage, double* s_loss, unsigned* s_flag) {
  constexpr int W1S = P::W1S;
  constexpr int NL = P::NL;
  const MlpDev w = mlp_dev(a.mlp);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float* st = s_stage + wv * 64 * TST;
  float* row = st + lane * TST;
  const int jj = lane & 31, hi = lane >> 5;
  const bool wgrad = a.want_wgrad != 0;
  const float sigma = a.sigma;
  const int rows = opaque(H);
  // FeatureOctree.set_zero (model/feature_octree.py:78-81, called at the top of query_feature): the trash row of every level is
  // re-zeroed here — the optimiser steps it like any row; nothing in this kernel reads it (a miss contributes nothing)
  if (blockIdx.x == 0 && tid < L * F) const_cast<float*>(a.ls.lv[tid / F].feat)[a.ls.lv[tid / F].rows * F + (tid % F)] = 0.f;

  long long ns = 0;
  float escale = 0.f;  // weight_e / n_surf
  if (EIK) {
    for (int p = 0; p < a.n_parts; ++p) ns += a.n_surf[p];
    escale = ns > 0 ? a.weight_e / (float)ns : 0.f;
  }

  float accW2[16], accW1[4];
  float accX = 0.f;  // hi == 0: dW1[jj][8] (w_t's column); hi == 1: db1[jj]
  float accw3 = 0.f, accb2 = 0.f, accb3 = 0.f;
  double acc[NL];  // [0] the main loss, [1] the eikonal term
#pragma unroll
  for (int q = 0; q < NL; ++q) acc[q] = 0.0;
#pragma unroll
  for (int q = 0; q < 16; ++q) accW2[q] = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) accW1[q] = 0.f;

  const long long tiles = P::tiles(a);
  for (long long t = (long long)blockIdx.x * kWaves + wv; t < tiles; t += (long long)gridDim.x * kWaves) {
    long long r = 0, j = 0;  // batch position, source row
    typename P::Lane ln = {};
    const bool valid = P::locate(a, t, lane, r, j, ln);
    float x0 = 0.f, x1 = 0.f, x2 = 0.f;
    bool surf = false;
    if (valid) {
      const float* c = a.coord + j * a.cstride;
      x0 = c[0], x1 = c[1], x2 = c[2];
      P::load(a, j, ln);
      if (EIK) surf = a.weight[j * a.wstride] > 0.f;
    }
    // ---- query: f (and A = d f / d x) over the levels the point hits; a padding lane misses everywhere
    float f[F];
    float A[EIK ? F : 1][3];
#pragma unroll
    for (int q = 0; q < F; ++q) f[q] = 0.f;
    if constexpr (EIK) {
#pragma unroll
      for (int q = 0; q < F; ++q) A[q][0] = A[q][1] = A[q][2] = 0.f;
    }
    int slot[L];
#pragma unroll
    for (int s = 0; s < L; ++s) slot[s] = valid ? level_slot(a.ls.lv[s], x0, x1, x2) : -1;
#pragma unroll
    for (int s = 0; s < L; ++s) {
      const LevelDev& Lv = a.ls.lv[s];
      if (slot[s] >= 0) {
        int ids[8];
        corner_ids(Lv.vals, (unsigned int)slot[s], ids);
        const Axis X = axis_weight<POLY>(x0, Lv.res, Lv.dres), Y = axis_weight<POLY>(x1, Lv.res, Lv.dres),
                   Z = axis_weight<POLY>(x2, Lv.res, Lv.dres);
        float wc[8];
        corner_weights(X.t, Y.t, Z.t, wc);
        float dw[8][3];
        if constexpr (EIK) corner_weight_grads(X, Y, Z, dw);
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) {
          const float4* rp = reinterpret_cast<const float4*>(Lv.feat + (long long)ids[cc] * F);
          const float4 r0 = rp[0], r1 = rp[1];
          const float rr[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
#pragma unroll
          for (int q = 0; q < F; ++q) {
            f[q] = fmaf(wc[cc], rr[q], f[q]);
            if constexpr (EIK) {
              A[q][0] = fmaf(dw[cc][0], rr[q], A[q][0]);
              A[q][1] = fmaf(dw[cc][1], rr[q], A[q][1]);
              A[q][2] = fmaf(dw[cc][2], rr[q], A[q][2]);
            }
          }
        }
      }
    }
    // ---- the head forward, rolled over the weight rows: h1 through the lane's LDS row into registers, h2 left at row[R_H2..),
    //      and v1 = W2^T (m2 .* w3) on the same pass over W2
    unsigned m1 = 0u, m2 = 0u;
TERM_ROW_LOOP(4)
    for (int k = 0; k < rows; ++k) {
      float z;
      if constexpr (P::SHIFT) z = fmaf(w.W1[k * W1S + F], P::shift(ln), w.B1[k]);  // a per-point shift of the first bias
      else z = w.B1[k];
#pragma unroll
      for (int q = 0; q < F; ++q) z = fmaf(w.W1[k * W1S + q], f[q], z);
      m1 |= (z > 0.f ? 1u : 0u) << k;
      row[k] = fmaxf(z, 0.f);
    }
    wave_lds_fence();
    float h1[H], v1[H];
#pragma unroll
    for (int k = 0; k < H; ++k) h1[k] = row[k], v1[k] = 0.f;
    wave_lds_fence();
    float y = w.B3[0];
TERM_ROW_LOOP(2)
    for (int jx = 0; jx < rows; ++jx) {
      float z = w.B2[jx];
#pragma unroll
      for (int k = 0; k < H; ++k) z = fmaf(w.W2[jx * H + k], h1[k], z);
      const bool on = z > 0.f;
      m2 |= (on ? 1u : 0u) << jx;
      const float h2 = on ? z : 0.f;
      row[R_H2 + jx] = h2;
      y = fmaf(w.W3[jx], h2, y);
      const float v2 = on ? w.W3[jx] : 0.f;
#pragma unroll
      for (int k = 0; k < H; ++k) v1[k] = fmaf(w.W2[jx * H + k], v2, v1[k]);
    }
    // v1 = m1 .* (...), left at row[0,32): where the first contraction phase reads it
#pragma unroll
    for (int k = 0; k < H; ++k) row[k] = ((m1 >> k) & 1u) ? v1[k] : 0.f;
    wave_lds_fence();
    float J[F];
#pragma unroll
    for (int q = 0; q < F; ++q) J[q] = 0.f;
TERM_ROW_LOOP(8)
    for (int k = 0; k < rows; ++k) {
      const float vk = row[k];
#pragma unroll
      for (int q = 0; q < F; ++q) J[q] = fmaf(w.W1[k * W1S + q], vk, J[q]);
    }
    // ---- the loss: delta = d main / d pred (the policy's), q = d (weight_e eik) / d g
    const float delta = P::delta(a, ln, valid, lane, y, st, acc);
    if (valid) P::store(a, r, y, delta);
    float qv[3] = {0.f, 0.f, 0.f};
    if (valid) {
      if constexpr (EIK) if (surf) {
        float g[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < F; ++q) {
          g[0] = fmaf(J[q], A[q][0], g[0]);
          g[1] = fmaf(J[q], A[q][1], g[1]);
          g[2] = fmaf(J[q], A[q][2], g[2]);
        }
        g[0] *= sigma, g[1] *= sigma, g[2] *= sigma;
        const float gn = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
        const float e = 1.0f - gn;
        acc[1] += (double)(e * e);
        const float coef = gn > 0.f ? (-2.0f * e / gn) * escale : 0.f;  // the guard: |g| = 0 contributes 1, no gradient
        qv[0] = coef * g[0], qv[1] = coef * g[1], qv[2] = coef * g[2];
      }
    }
    const bool live = EIK && (qv[0] != 0.f || qv[1] != 0.f || qv[2] != 0.f);  // a row with a second-order gradient
    if (wgrad) {
      // ---- second-order pieces behind `live`: r = sigma A q, a1 = m1 .* (W1f r) (through row[32..64) into registers),
      //      a2 = m2 .* (W2 a1) added to delta h2 in place; h1 becomes u = delta h1 + a1
      float rq[F];
#pragma unroll
      for (int q = 0; q < F; ++q) rq[q] = 0.f;
      bool second = false;
      if constexpr (EIK) {
        if (live) {
          second = true;
#pragma unroll
          for (int q = 0; q < F; ++q) rq[q] = sigma * (A[q][0] * qv[0] + A[q][1] * qv[1] + A[q][2] * qv[2]);
TERM_ROW_LOOP(4)
          for (int k = 0; k < rows; ++k) {
            float tt = 0.f;
#pragma unroll
            for (int q = 0; q < F; ++q) tt = fmaf(w.W1[k * W1S + q], rq[q], tt);
            row[32 + k] = ((m1 >> k) & 1u) ? tt : 0.f;
          }
          wave_lds_fence();
          float a1[H];
#pragma unroll
          for (int k = 0; k < H; ++k) a1[k] = row[32 + k];
          wave_lds_fence();
TERM_ROW_LOOP(2)
          for (int jx = 0; jx < rows; ++jx) {
            float tt = 0.f;
#pragma unroll
            for (int k = 0; k < H; ++k) tt = fmaf(w.W2[jx * H + k], a1[k], tt);
            row[R_H2 + jx] = fmaf(delta, row[R_H2 + jx], ((m2 >> jx) & 1u) ? tt : 0.f);
          }
#pragma unroll
          for (int k = 0; k < H; ++k) h1[k] = fmaf(delta, h1[k], a1[k]);
        }
      }
      if (!second) {
#pragma unroll
        for (int k = 0; k < H; ++k) row[R_H2 + k] *= delta;
#pragma unroll
        for (int k = 0; k < H; ++k) h1[k] *= delta;
      }
      // ---- first contraction phase: [0,32) v1 | [32,40) delta f + r | [40] delta ts | [41] delta | [65,97) delta h2 + a2
#pragma unroll
      for (int q = 0; q < F; ++q) row[32 + q] = fmaf(delta, f[q], rq[q]);
      if constexpr (P::SHIFT) row[R_TS] = delta * P::shift(ln);
      else row[R_TS] = 0.f;
      row[R_D1] = delta;
      wave_lds_fence();
TERM_ROW_LOOP(4)
      for (int pp = 0; pp < 64; ++pp) {
        const float* pr = st + pp * TST;
        const float l = pr[jj];
#pragma unroll
        for (int q = 0; q < 4; ++q) accW1[q] = fmaf(l, pr[32 + hi * 4 + q], accW1[q]);  // dW1f += v1 (x) (delta f + r)
        accX = fmaf(l, pr[R_TS + hi], accX);                                           // dW1[:,8] / db1
        accw3 += pr[R_H2 + jj];                                                        // dw3 += delta h2 + a2
        accb3 += pr[R_D1];                                                             // db3 += delta
      }
      wave_lds_fence();
      // ---- second phase: [0,32) v2 = m2 .* w3 | [32,64) u = delta h1 + a1 | [64] delta
#pragma unroll
      for (int jx = 0; jx < H; ++jx) row[jx] = ((m2 >> jx) & 1u) ? w.W3[jx] : 0.f;
#pragma unroll
      for (int k = 0; k < H; ++k) row[32 + k] = h1[k];
      row[R_D2] = delta;
      wave_lds_fence();
TERM_ROW_LOOP(4)
      for (int pp = 0; pp < 64; ++pp) {
        const float* pr = st + pp * TST;
        const float l = pr[jj];
#pragma unroll
        for (int q = 0; q < 16; ++q) accW2[q] = fmaf(l, pr[32 + hi * 16 + q], accW2[q]);  // dW2 += v2 (x) u
        accb2 = fmaf(l, pr[R_D2], accb2);                                                 // db2 += delta v2
      }
      wave_lds_fence();
    }
    // ---- feature grads: rows += (w_c delta + sigma dw_c/dx . q) J
    float gval[8];
    stage_row_grads(st, lane, J, gval);
#pragma unroll
    for (int s = 0; s < L; ++s) {
      const LevelDev& Lv = a.ls.lv[s];
      if (!Lv.grad) continue;  // (wave-uniform)
      const bool hit = slot[s] >= 0;
      int ids[8];
      corner_ids(Lv.vals, hit ? (unsigned int)slot[s] : 0u, ids);
      const Axis X = axis_weight<POLY>(x0, Lv.res, Lv.dres), Y = axis_weight<POLY>(x1, Lv.res, Lv.dres),
                 Z = axis_weight<POLY>(x2, Lv.res, Lv.dres);
      float cf[8];  // w_c delta + sigma (d w_c / d x . q): what corner c's row receives, times J
      corner_weights(X.t, Y.t, Z.t, cf);
#pragma unroll
      for (int c = 0; c < 8; ++c) cf[c] *= delta;
      if constexpr (EIK) {
        float dw[8][3];
        corner_weight_grads(X, Y, Z, dw);
#pragma unroll
        for (int c = 0; c < 8; ++c) cf[c] = fmaf(sigma, dw[c][0] * qv[0] + dw[c][1] * qv[1] + dw[c][2] * qv[2], cf[c]);
      }
      scatter_corner_rows(Lv, ids, hit, valid && !hit, cf, J, gval, lane);
    }
  }

  // ---- the workgroup's partial: its waves summed in index order through LDS
#pragma unroll
  for (int q = 0; q < NL; ++q) acc[q] = wave_sum_d(acc[q]);
  __syncthreads();
  constexpr int NV = 24;
  float vals[NV];
#pragma unroll
  for (int q = 0; q < 16; ++q) vals[q] = accW2[q];
#pragma unroll
  for (int q = 0; q < 4; ++q) vals[16 + q] = accW1[q];
  vals[20] = accX, vals[21] = accw3, vals[22] = accb2, vals[23] = accb3;
  if (wgrad) {
#pragma unroll
    for (int v = 0; v < NV; ++v) s_stage[(wv * NV + v) * 64 + lane] = vals[v];
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < NL; ++q) s_loss[NL * wv + q] = acc[q];
  }
  __syncthreads();
  if (wv == 0) {
    if (wgrad) {
      float* mine = a.part + (size_t)blockIdx.x * PW;
#pragma unroll
      for (int ww = 1; ww < kWaves; ++ww) {
#pragma unroll
        for (int v = 0; v < NV; ++v) vals[v] += s_stage[(ww * NV + v) * 64 + lane];
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) mine[P_W2 + jj * H + hi * 16 + q] = vals[q];
#pragma unroll
      for (int q = 0; q < 4; ++q) mine[P_W1 + jj * F + hi * 4 + q] = vals[16 + q];
      if (P::SHIFT || hi) mine[(hi ? P_B1 : P_WT) + jj] = vals[20];
      if (hi == 0) {
        mine[P_W3 + jj] = vals[21];
        mine[P_B2 + jj] = vals[22];
      }
      if (lane == 0) mine[P_B3] = vals[23];
    }
    if (lane < NL) {
      double s = s_loss[lane];
#pragma unroll
      for (int ww = 1; ww < kWaves; ++ww) s += s_loss[NL * ww + lane];
      a.lpart[(size_t)blockIdx.x * NL + lane] = s;
    }
  }
  point_grid_sum<P>(a, wgrad, ns, s_flag);
}

}  // namespace pstep
}  // namespace shine
