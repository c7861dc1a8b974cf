// shine_time_step.hip — one training iteration's forward + backward of a TIME-CONDITIONED map in ONE launch (the drivers' loop
// body with config.time_conditioned, shine_batch.py:119-130,141-142,172-185,208-209):
//
//   f      = query_feature(coord)                          levels summed, a miss contributes nothing; set_zero: the trash rows of
//                                                          the feature tables are re-zeroed by the launch
//   pred   = w3 . relu(W2 relu(W1f f + (b1 + w_t ts)) + b2) + b3          W1 = [W1f | w_t] read in place, row stride 9 (3.20)
//   bce    = BCEWithLogits(pred, sigmoid(label / sigma))   'mean' (/ n_global) or 'sum'
//   eik    = mean over weight > 0 of (1 - |g|)^2,  g = sigma d pred / d coord      (EIK builds; 0 without a surface row)
//   loss   = bce + weight_e * eik
//   grads += d loss / d {feature tables, W1, b1, W2, b2, w3, b3}
//
// One wave = one tile of 64 batch rows at a time, lane = row (k_sem_step's launch shape).  The head has ONE output, so its
// first-order backward is delta = d bce / d pred times the Jacobian chain the eikonal term needs anyway:
//   v2 = m2 .* w3,  v1 = m1 .* (W2^T v2),  J = W1f^T v1 = d pred / d f;   d2 = delta v2,  d1 = delta v1,  d f = delta J
// and with the eikonal term's second-order pieces (q = d loss / d g; r = sigma A q, a1 = m1 .* (W1f r), a2 = m2 .* (W2 a1),
// shine_gterm_body.hpp's chain with delta = 0) every weight gradient is ONE contraction over the tile's 64 staged rows:
//   dW1f += v1 (x) (delta f + r)     dW1[:,8] += v1 . (delta ts)     db1 += v1 . delta
//   dW2  += v2 (x) (delta h1 + a1)   db2 += v2 . delta               dw3 += delta h2 + a2      db3 += delta
// (the second-order part reaches W1f, W2 and w3 only: J depends on w_t, ts and the biases through the ReLU masks alone).
// Feature rows receive (w_c delta + sigma dw_c/dx . q) J with the lanes transposed to (row, feature) as in k_sem_step — one fp32
// atomic instruction covers 8 rows x the 8 features of a corner; the misses of a wave reach the trash row as one atomic per
// feature.  The decoder layers are rolled loops over weight rows with scalar loads (3.18).
//
// The six weight grads and both loss sums (BCE over the batch, eikonal over the surface rows, fp64 from the lanes up) are
// added in a fixed order inside a wave and a workgroup and in two ticket levels across workgroups (shine_arrive.hpp), so they
// are bit-identical from call to call; the workgroup that finishes the sum ADDS the grads, writes the loss and leaves the
// workspace all zero.
#include "shine_arrive.hpp"
#include "shine_term_host.hpp"

namespace shine {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;  // waves of a workgroup, a tile each
constexpr int kMaxBlocks = 256;
constexpr int kGroup = 16;  // workgroups per first-level run
constexpr int kGroups = kMaxBlocks / kGroup;
constexpr int F9 = F + 1;  // row stride of W1 = [W1f | w_t]
// a lane's staging row (floats): [0,32) left operand | [32,64) right operand ([40] delta ts, [41] delta beside the 8-wide one)
// | [64] delta | [65,97) h2, then delta h2 + a2
constexpr int TST = 97;  // (odd: conflict-free column reads)
constexpr int R_TS = 40, R_D1 = 41, R_D2 = 64, R_H2 = 65;
// partial layout (floats): W1f [32][8] | w_t [32] | b1 [32] | W2 [32][32] | b2 [32] | w3 [32] | b3 [1] + 3 unused
constexpr int P_W1 = 0, P_WT = P_W1 + H * F, P_B1 = P_WT + H, P_W2 = P_B1 + H, P_B2 = P_W2 + H * H, P_W3 = P_B2 + H,
              P_B3 = P_W3 + H, PW = P_B3 + 4;
static_assert((kGroups + 1) * sizeof(unsigned) <= 256 && PW % 4 == 0, "layout");
static_assert(kGroup <= 32 && kGroups <= 32, "a run's two loss partials are read by one wave, a lane each");

#define TIME_LOOP_STR(x) #x
#define TIME_ROW_LOOP(n) _Pragma(TIME_LOOP_STR(clang loop vectorize(disable) interleave(disable) unroll_count(n)))

struct TimeStepArgs {
  LevelSet ls;
  const float* coord;   // rows of `cstride` floats, x y z first
  const int* idx;       // [n] gather or null
  const float* label;   // rows of `lstride` floats
  const float* weight;  // rows of `wstride` floats (EIK builds)
  const float* ts;      // indexed like coord
  const long long* n_surf;
  long long n;
  int cstride, lstride, wstride;
  int n_parts;  // entries of n_surf to add up (>= 1)
  int reduction_sum;
  float sigma, inv_n, weight_e;
  const float* mlp[6];
  float* gW1;  // [32][9]
  float* gW2;
  float* gw3;
  float* gb1;
  float* gb2;
  float* gb3;
  int want_wgrad;
  float* pred;  // [n] at the batch position, or null
  float* loss_out;
  // the workspace's arrays: tickets ([0] run level, [1..kGroups] first level) | part [kMaxBlocks][PW] | run [kGroups][PW] |
  // loss_part [kMaxBlocks][2] | loss_run [kGroups][2]
  unsigned* cnt;
  float* part;
  float* run;
  double* lpart;
  double* lrun;
};

struct TimeWork {
  unsigned* cnt;
  float *part, *run;
  double *lpart, *lrun;
  size_t bytes;
};
TimeWork time_layout(void* workspace) {
  Arena ar(workspace);
  TimeWork w;
  w.cnt = ar.take<unsigned>(64);
  w.part = ar.take<float>((size_t)kMaxBlocks * PW);
  w.run = ar.take<float>((size_t)kGroups * PW);
  w.lpart = ar.take<double>((size_t)kMaxBlocks * 2);
  w.lrun = ar.take<double>((size_t)kGroups * 2);
  w.bytes = ar.bytes();
  return w;
}

// where entry k of the partial layout is added: W1's rows are 9 floats apart and its ninth column is w_t's
__device__ __forceinline__ float* time_grad_dst(const TimeStepArgs& a, int k) {
  if (k < P_WT) return a.gW1 + (k >> 3) * F9 + (k & 7);
  if (k < P_B1) return a.gW1 + (k - P_WT) * F9 + F;
  if (k < P_W2) return a.gb1 + (k - P_B1);
  if (k < P_B2) return a.gW2 + (k - P_W2);
  if (k < P_W3) return a.gb2 + (k - P_B2);
  if (k < P_B3) return a.gw3 + (k - P_W3);
  return k == P_B3 ? a.gb3 : nullptr;
}

// The sum over the grid of the workgroups' partials, gterm_grid_sum's two ticket levels with six tensors and two loss sums: the
// last workgroup of each run of kGroup to arrive sums that run in index order, the last run to finish sums the run sums in
// index order, ADDS them to the six tensors and writes the loss.  Whoever sums a partial clears it behind itself and the tickets
// are reset, so the whole workspace is zero again when the launch ends.
__device__ __forceinline__ void time_grid_sum(const TimeStepArgs& a, bool wgrad, long long ns, unsigned* verdict) {
  const unsigned G = gridDim.x;
  const unsigned grp = blockIdx.x / kGroup;
  const unsigned g0 = grp * kGroup;
  const unsigned gsz = (G - g0) < (unsigned)kGroup ? (G - g0) : (unsigned)kGroup;
  const unsigned ngrp = (G + kGroup - 1) / kGroup;
  const unsigned lane = threadIdx.x & 63u;
  const unsigned li = lane >> 1, lc = lane & 1u;  // (partial, which of its two sums)

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
    const double v = li < gsz ? a.lpart[(size_t)(g0 + li) * 2 + lc] : 0.0;
    if (li < gsz) a.lpart[(size_t)(g0 + li) * 2 + lc] = 0.0;
    double s = 0.0;
    for (unsigned b = 0; b < (unsigned)kGroup; ++b) s += __shfl(v, (int)(2 * b + lc), 64);
    if (lane < 2) a.lrun[(size_t)grp * 2 + lc] = s;
  }
  if (threadIdx.x == 0) __hip_atomic_store(a.cnt + 1 + grp, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // for the next call

  if (!arrive_last(a.cnt, ngrp, verdict)) return;
  if (wgrad) {
    for (int k = threadIdx.x; k <= P_B3; k += kThreads) {
      float s = 0.f;
      for (unsigned r = 0; r < ngrp; ++r) s += a.run[(size_t)r * PW + k];
      float* dst = time_grad_dst(a, k);
      dst[0] += s;
    }
    __syncthreads();  // (every read of the run sums is done before they are cleared)
    for (int c = threadIdx.x; c < PW / 4; c += kThreads)
      for (unsigned r = 0; r < ngrp; ++r) *reinterpret_cast<float4*>(a.run + (size_t)r * PW + 4 * c) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (threadIdx.x < 64) {
    const double v = li < ngrp ? a.lrun[(size_t)li * 2 + lc] : 0.0;
    if (li < ngrp) a.lrun[(size_t)li * 2 + lc] = 0.0;
    double s = 0.0;
    for (unsigned r = 0; r < (unsigned)kGroups; ++r) s += __shfl(v, (int)(2 * r + lc), 64);
    const double es = __shfl(s, 1, 64);  // lane 1: the eikonal sum
    if (lane == 0) {
      const double bce = a.reduction_sum ? s : s * (double)a.inv_n;
      const double eik = ns > 0 ? es / (double)ns : 0.0;
      a.loss_out[0] = (float)(bce + (double)a.weight_e * eik);
    }
  }
  if (threadIdx.x == 0) __hip_atomic_store(a.cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int L, bool POLY, bool EIK>
__global__ __launch_bounds__(kThreads) void k_time_step(const TimeStepArgs a) {
  __shared__ float s_stage[kWaves * 64 * TST];
  __shared__ double s_loss[kWaves * 2];
  __shared__ unsigned s_flag;
  const MlpDev w = mlp_dev(a.mlp);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float* st = s_stage + wv * 64 * TST;
  float* row = st + lane * TST;
  const int jj = lane & 31, hi = lane >> 5;
  const int sub = lane >> 3, fi = lane & 7;
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
  double accbce = 0.0, acceik = 0.0;
#pragma unroll
  for (int q = 0; q < 16; ++q) accW2[q] = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) accW1[q] = 0.f;

  const long long tiles = (a.n + 63) >> 6;
  for (long long t = (long long)blockIdx.x * kWaves + wv; t < tiles; t += (long long)gridDim.x * kWaves) {
    const long long r = t * 64 + lane;  // batch position
    const bool valid = r < a.n;
    float x0 = 0.f, x1 = 0.f, x2 = 0.f, ts = 0.f, label = 0.f;
    bool surf = false;
    if (valid) {
      const long long j = a.idx ? (long long)a.idx[r] : r;
      const float* c = a.coord + j * a.cstride;
      x0 = c[0], x1 = c[1], x2 = c[2];
      label = a.label[j * a.lstride];
      ts = a.ts[j];
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
TIME_ROW_LOOP(4)
    for (int k = 0; k < rows; ++k) {
      float z = fmaf(w.W1[k * F9 + F], ts, w.B1[k]);  // the time input: a per-point shift of the first bias
#pragma unroll
      for (int q = 0; q < F; ++q) z = fmaf(w.W1[k * F9 + q], f[q], z);
      m1 |= (z > 0.f ? 1u : 0u) << k;
      row[k] = fmaxf(z, 0.f);
    }
    wave_lds_fence();
    float h1[H], v1[H];
#pragma unroll
    for (int k = 0; k < H; ++k) h1[k] = row[k], v1[k] = 0.f;
    wave_lds_fence();
    float y = w.B3[0];
TIME_ROW_LOOP(2)
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
TIME_ROW_LOOP(8)
    for (int k = 0; k < rows; ++k) {
      const float vk = row[k];
#pragma unroll
      for (int q = 0; q < F; ++q) J[q] = fmaf(w.W1[k * F9 + q], vk, J[q]);
    }
    if (valid && a.pred) a.pred[r] = y;
    // ---- the loss: delta = d bce / d pred, q = d (weight_e eik) / d g
    float delta = 0.f;
    float qv[3] = {0.f, 0.f, 0.f};
    if (valid) {
      const float zt = sigmoidf_acc(label / sigma);
      accbce += (double)(fmaxf(y, 0.f) - y * zt + log1pf(expf(-fabsf(y))));
      delta = (sigmoidf_acc(y) - zt) * a.inv_n;
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
        acceik += (double)(e * e);
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
TIME_ROW_LOOP(4)
          for (int k = 0; k < rows; ++k) {
            float tt = 0.f;
#pragma unroll
            for (int q = 0; q < F; ++q) tt = fmaf(w.W1[k * F9 + q], rq[q], tt);
            row[32 + k] = ((m1 >> k) & 1u) ? tt : 0.f;
          }
          wave_lds_fence();
          float a1[H];
#pragma unroll
          for (int k = 0; k < H; ++k) a1[k] = row[32 + k];
          wave_lds_fence();
TIME_ROW_LOOP(2)
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
      row[R_TS] = delta * ts;
      row[R_D1] = delta;
      wave_lds_fence();
TIME_ROW_LOOP(4)
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
TIME_ROW_LOOP(4)
      for (int pp = 0; pp < 64; ++pp) {
        const float* pr = st + pp * TST;
        const float l = pr[jj];
#pragma unroll
        for (int q = 0; q < 16; ++q) accW2[q] = fmaf(l, pr[32 + hi * 16 + q], accW2[q]);  // dW2 += v2 (x) u
        accb2 = fmaf(l, pr[R_D2], accb2);                                                 // db2 += delta v2
      }
      wave_lds_fence();
    }
    // ---- feature grads: J through LDS once ([row][feature] -> lane (row & 7 group, feature)), ids and weights by shuffle
#pragma unroll
    for (int q = 0; q < F; ++q) st[lane * F + q] = J[q];
    wave_lds_fence();
    float gval[8];
#pragma unroll
    for (int G = 0; G < 8; ++G) gval[G] = st[G * 64 + lane];
    wave_lds_fence();
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
      // a miss: all eight corners address the trash row, which receives sum_c of the same terms — one atomic per wave and feature
      const bool miss = valid && !hit;
      if (__any(miss)) {
        const float cm = miss ? csum : 0.f;
#pragma unroll
        for (int q = 0; q < F; ++q) {
          const float tsum = wave_sum(cm * J[q]);
          if (lane == 0 && tsum != 0.f) atomic_add_f32(Lv.grad + Lv.rows * F + q, tsum);
        }
      }
    }
  }

  // ---- the workgroup's partial: its waves summed in index order through LDS
  accbce = wave_sum_d(accbce);
  acceik = wave_sum_d(acceik);
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
  if (lane == 0) s_loss[2 * wv] = accbce, s_loss[2 * wv + 1] = acceik;
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
      mine[(hi ? P_B1 : P_WT) + jj] = vals[20];
      if (hi == 0) {
        mine[P_W3 + jj] = vals[21];
        mine[P_B2 + jj] = vals[22];
      }
      if (lane == 0) mine[P_B3] = vals[23];
    }
    if (lane < 2) {
      double s = s_loss[lane];
#pragma unroll
      for (int ww = 1; ww < kWaves; ++ww) s += s_loss[2 * ww + lane];
      a.lpart[(size_t)blockIdx.x * 2 + lane] = s;
    }
  }
  time_grid_sum(a, wgrad, ns, &s_flag);
}

// Launch shape: k_sem_step's — four waves per workgroup, a tile each, at most kMaxBlocks workgroups with a grid stride past
// 64 K rows; it depends on the tile count alone, so equal batches sum in equal order.
unsigned time_step_blocks(long long tiles) {
  const long long b = (tiles + kWaves - 1) / kWaves;
  return (unsigned)(b > kMaxBlocks ? kMaxBlocks : b);
}

}  // namespace
}  // namespace shine

using namespace shine;

extern "C" int shine_time_step(const shine_tables* t, const shine_step_config* cfg, const float* coord, int32_t coord_stride,
                               const int32_t* idx, const float* label, const float* weight, int32_t weight_stride,
                               const float* ts, const int64_t* n_surf, int32_t n_surf_parts, int64_t n,
                               const float* const* feats, const int64_t* rows, float* const* grad_feats,
                               const float* const* mlp, float* const* grad_mlp, float* pred_out, float* loss_out,
                               void* workspace, size_t* workspace_bytes, void* stream) {
  static const char* const kEntry = "shine_time_step";
  if (!workspace_bytes) return term_refuse(kEntry, "null workspace_bytes");
  const TimeWork wk = time_layout(workspace);
  if (!workspace) {  // the size query (one layout for every batch: the workgroup count is capped)
    *workspace_bytes = wk.bytes;
    return SHINE_OK;
  }
  TimeStepArgs a = {};
  int rc = term_prologue(kEntry, t, cfg, coord_stride, n, feats, rows, loss_out, workspace);
  if (rc == SHINE_OK) rc = term_decoder(kEntry, mlp, grad_mlp, &a);
  if (rc != SHINE_OK) return rc;
  SHINE_WORKSPACE_FITS(wk.bytes, workspace, *workspace_bytes, "shine_time_step");
  if (cfg->loss_weight_on) return term_refuse(kEntry, "loss_weight_on is not served (False in every shipped config)");
  if (n >= (1ll << 31)) return term_refuse(kEntry, "n exceeds 2^31 - 1 rows");
  const bool eik = cfg->eikonal_on != 0;
  if (eik && weight_stride != 1 && weight_stride != 8)
    return term_refuse(kEntry, "weight_stride is 1 (an array) or 8 (32-byte pool records)");
  if (n_surf_parts < 0 || n_surf_parts > 64) return term_refuse(kEntry, "n_surf_parts is 0 .. 64");
  if (n > 0 && (!coord || !ts || (coord_stride == 3 && !label) || (eik && (!weight || !n_surf))))
    return term_refuse(kEntry, "null argument");
  rc = term_levels(kEntry, t, cfg, feats, rows, grad_feats, &a.ls);
  if (rc != SHINE_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) return term_empty(loss_out, st);
  if (grad_mlp) a.gb1 = grad_mlp[1], a.gb2 = grad_mlp[3], a.gb3 = grad_mlp[5];
  a.coord = coord;
  a.idx = idx;
  a.label = coord_stride == 8 ? coord + 3 : label;  // dword 3 of a pool record
  a.lstride = coord_stride == 8 ? 8 : 1;
  a.weight = weight;
  a.wstride = weight_stride;
  a.ts = ts;
  a.n_surf = reinterpret_cast<const long long*>(n_surf);
  a.n_parts = n_surf_parts > 1 ? n_surf_parts : 1;
  a.n = n;
  a.cstride = coord_stride;
  a.reduction_sum = cfg->reduction_sum;
  a.sigma = cfg->sigma;
  a.inv_n = (float)cfg->inv_n;
  a.weight_e = cfg->weight_e;
  a.pred = pred_out;
  a.loss_out = loss_out;
  a.cnt = wk.cnt, a.part = wk.part, a.run = wk.run, a.lpart = wk.lpart, a.lrun = wk.lrun;
  const dim3 grid(time_step_blocks((n + 63) / 64));
  dispatch_levels_poly(cfg->n_levels, cfg->poly_int_on != 0, [&](auto l, auto p) {
    constexpr int LL = decltype(l)::value;
    constexpr bool PP = decltype(p)::value;
    if (eik)
      hipLaunchKernelGGL((k_time_step<LL, PP, true>), grid, dim3(kThreads), 0, st, a);
    else
      hipLaunchKernelGGL((k_time_step<LL, PP, false>), grid, dim3(kThreads), 0, st, a);
  });
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}
