// shine_gterm_body.hpp — the ONE chain of the training terms that are a loss on g = d pred / d coord (the surface-normal term,
// shine_normal_step.hip; the gradient-consistency term, shine_consistency_step.hip): the closed-form g of a lane's point, the
// term's q = dL/dg, and the second-order backward of that loss into the feature tables and W1, W2, w3.
//
// One wave = one tile of 64 lanes at a time, lane = point (k_sem_step's launch shape and LDS staging, [64][ST] floats per wave);
// the per-point math is k_step_v0's lane-per-point chain, its loops over weight rows ROLLED with scalar loads as in k_sem_step
// (fully unrolled with the weights in LDS it took 256 VGPRs + 256 AGPRs + 1.2 KB of scratch: DESIGN.md 3.18).  Second-order
// backward with delta = 0: r = A q, a1 = m1 .* (W1 r), a2 = m2 .* (W2 a1); dW1 += v1 (x) r, dW2 += v2 (x) a1, dw3 += a2 by
// contract64r over the staged tile; feature rows += (dw_c/dx . q) J with the lanes transposed to (row, feature) as in k_sem_step
// — one fp32 atomic instruction covers 8 rows x the 8 features of a corner.
//
// The three weight grads and the loss are summed in a fixed order inside a wave and a workgroup and in two ticket levels
// across workgroups (shine_arrive.hpp), so they are bit-identical from call to call; the workgroup that finishes the sum ADDS
// them to grad_mlp and writes the loss.  The loss is summed in fp64 from the lanes up and divided by the term's count in fp64.
//
// A kernel instantiates gterm_step<L, POLY, P> with a POLICY P that says what a lane's point is, what the term is and what it
// is divided by:
//   P::Args                      the kernel's argument struct; the chain reads ls, mlp, gW1 / gW2 / gw3, want_wgrad, loss_out, ws
//   P::Ctx, P::begin(a)          per-thread launch facts, read once; Ctx has `den` (the term's count, long long) and `scale`
//                                (weight / den, what q is multiplied by)
//   P::tiles(a)                  tiles of 64 lanes
//   P::select(a, cx, t, lane, j, ln)   does the lane have a point in tile t -> bool; j = its row, ln (P::Lane) = what load / term need
//   P::load(a, j, lane, x0, x1, x2, ln)  the point's coordinates (called by the lanes select() accepted)
//   P::term(g, ln, lane, scale, q)       -> the lane's addend to the loss sum; q = d (weight * loss) / d g of the lane's point
//                                (q == 0: the lane sits out of the backward).  Called by every accepted lane of the wave at once
//   P::kFlags                    the kernel marks a.touched[s][row] = 1 for every corner row a live lane scatters to
//   P::finish(a, cx)             called by thread 0 of the workgroup that finished the grid sum, after the loss is written
#pragma once
#include "shine_arrive.hpp"
#include "shine_internal.hpp"

namespace shine {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;  // waves of a workgroup, a tile each
constexpr int kMaxBlocks = 256;
constexpr int kGroup = 16;  // workgroups per first-level run
constexpr int kGroups = kMaxBlocks / kGroup;
// partial layout (floats): W1 [32][8] | W2 [32][32] | w3 [32]
constexpr int P_W1 = 0, P_W2 = P_W1 + H * F, P_W3 = P_W2 + H * H, PW = P_W3 + H;
// workspace: counters ([0] run-level ticket, [1..kGroups] first-level tickets) | float part[kMaxBlocks][PW] | float run[kGroups][PW]
// | double loss_part[kMaxBlocks] | double loss_run[kGroups]
constexpr size_t kCounterBytes = 256;
constexpr size_t kPartOff = kCounterBytes;
constexpr size_t kRunOff = kPartOff + (size_t)kMaxBlocks * PW * sizeof(float);
constexpr size_t kLossOff = kRunOff + (size_t)kGroups * PW * sizeof(float);
constexpr size_t kLossRunOff = kLossOff + (size_t)kMaxBlocks * sizeof(double);
constexpr size_t kWorkspaceEnd = kLossRunOff + (size_t)kGroups * sizeof(double);
static_assert((kGroups + 1) * sizeof(unsigned) <= kCounterBytes && PW % 4 == 0 && kLossOff % 8 == 0, "layout");
static_assert(kGroup <= 64 && kGroups <= 64, "a run's loss partials are read by one wave, a lane each");

#define NRM_LOOP_STR(x) #x
#define NRM_ROW_LOOP(n) _Pragma(NRM_LOOP_STR(clang loop vectorize(disable) interleave(disable) unroll_count(n)))

// The sum over the grid of the workgroups' partials, sem_grid_sum's two ticket levels: the last workgroup of each run of kGroup
// to arrive sums that run in index order, the last run to finish sums the run sums in index order, ADDS them to the three
// tensors and writes the loss (the fp64 sum over `den`, 0 without one).  Called by every thread of every workgroup; whoever sums a
// partial clears it behind itself and the counters are reset, so the whole workspace is zero again when the launch ends.
// -> whether this workgroup finished the sum.
template <class Args>
__device__ __forceinline__ bool gterm_grid_sum(const Args& a, bool wgrad, long long ns, unsigned* verdict) {
  unsigned* cnt = reinterpret_cast<unsigned*>(a.ws);
  float* part = reinterpret_cast<float*>(a.ws + kPartOff);
  float* runsum = reinterpret_cast<float*>(a.ws + kRunOff);
  double* lpart = reinterpret_cast<double*>(a.ws + kLossOff);
  double* lrun = reinterpret_cast<double*>(a.ws + kLossRunOff);
  const unsigned G = gridDim.x;
  const unsigned grp = blockIdx.x / kGroup;
  const unsigned g0 = grp * kGroup;
  const unsigned gsz = (G - g0) < (unsigned)kGroup ? (G - g0) : (unsigned)kGroup;
  const unsigned ngrp = (G + kGroup - 1) / kGroup;
  const unsigned lane = threadIdx.x & 63u;

  if (!arrive_last(cnt + 1 + grp, gsz, verdict)) return false;
  if (wgrad) {
    for (int c = threadIdx.x; c < PW / 4; c += kThreads) {
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
      for (unsigned b = 0; b < gsz; ++b) {
        float4* src = reinterpret_cast<float4*>(part + (size_t)(g0 + b) * PW + 4 * c);
        const float4 v = *src;
        s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
        *src = make_float4(0.f, 0.f, 0.f, 0.f);  // (read once, by this thread: the workspace is left ALL zero)
      }
      *reinterpret_cast<float4*>(runsum + (size_t)grp * PW + 4 * c) = s;
    }
  }
  if (threadIdx.x < 64) {  // (a lane per partial: per-lane addresses, then a fixed-order sum over the lanes)
    const double v = lane < gsz ? lpart[g0 + lane] : 0.0;
    if (lane < gsz) lpart[g0 + lane] = 0.0;
    double s = 0.0;
    for (unsigned b = 0; b < (unsigned)kGroup; ++b) s += __shfl(v, (int)b, 64);
    if (lane == 0) lrun[grp] = s;
  }
  if (threadIdx.x == 0) __hip_atomic_store(cnt + 1 + grp, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // for the next call

  if (!arrive_last(cnt, ngrp, verdict)) return false;
  if (wgrad) {
    for (int c = threadIdx.x; c < PW / 4; c += kThreads) {
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
      for (unsigned r = 0; r < ngrp; ++r) {
        float4* src = reinterpret_cast<float4*>(runsum + (size_t)r * PW + 4 * c);
        const float4 v = *src;
        s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
        *src = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      const int k = 4 * c;
      float* dst = k < P_W2 ? a.gW1 + (k - P_W1) : k < P_W3 ? a.gW2 + (k - P_W2) : a.gw3 + (k - P_W3);
      dst[0] += s.x, dst[1] += s.y, dst[2] += s.z, dst[3] += s.w;  // (a caller's grad tensor may be a 4-byte aligned view)
    }
  }
  if (threadIdx.x < 64) {
    const double v = lane < ngrp ? lrun[lane] : 0.0;
    if (lane < ngrp) lrun[lane] = 0.0;
    double s = 0.0;
    for (unsigned r = 0; r < (unsigned)kGroups; ++r) s += __shfl(v, (int)r, 64);
    if (lane == 0) a.loss_out[0] = ns > 0 ? (float)(s / (double)ns) : 0.f;
  }
  if (threadIdx.x == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

// The kernel's body: s_stage [kWaves * 64 * ST] floats, s_loss [kWaves] doubles and s_flag are the kernel's LDS.
template <int L, bool POLY, class P>
__device__ __forceinline__ void gterm_step(const typename P::Args& a, float* s_stage, double* s_loss, unsigned* s_flag) {
  const MlpDev w = mlp_dev(a.mlp);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float* st = s_stage + wv * 64 * ST;
  float* row = st + lane * ST;
  const int jj = lane & 31, hi = lane >> 5;
  const int sub = lane >> 3, fi = lane & 7;
  const bool wgrad = a.want_wgrad != 0;

  const typename P::Ctx cx = P::begin(a);
  const long long ns = cx.den;
  const float scale = cx.scale;

  float accW2[16], accW1[4];
  float accw3 = 0.f;
  double accloss = 0.0;
#pragma unroll
  for (int q = 0; q < 16; ++q) accW2[q] = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) accW1[q] = 0.f;

  const long long tiles = P::tiles(a);
  for (long long t = (long long)blockIdx.x * kWaves + wv; t < tiles; t += (long long)gridDim.x * kWaves) {
    long long j = 0;
    typename P::Lane ln;
    const bool active = P::select(a, cx, t, lane, j, ln);
    if (!__any(active)) continue;  // a tile without a point (wave-uniform)

    float x0 = 0.f, x1 = 0.f, x2 = 0.f;
    float qv[3] = {0.f, 0.f, 0.f};
    float J[F];
#pragma unroll
    for (int q = 0; q < F; ++q) J[q] = 0.f;
    int slot[L];
#pragma unroll
    for (int s = 0; s < L; ++s) slot[s] = -1;
    bool live = false;  // a point with a gradient (q != 0)
    unsigned m2 = 0u;
    float a1[H];
#pragma unroll
    for (int k = 0; k < H; ++k) a1[k] = 0.f;

    if (active) {
      P::load(a, j, lane, x0, x1, x2, ln);
      // ---- query: f and A = d f / d x over the levels the point hits
      float f[F];
      float A[F][3];
#pragma unroll
      for (int q = 0; q < F; ++q) {
        f[q] = 0.f;
        A[q][0] = A[q][1] = A[q][2] = 0.f;
      }
#pragma unroll
      for (int s = 0; s < L; ++s) {
        const LevelDev& Lv = a.ls.lv[s];
        slot[s] = level_slot(Lv, x0, x1, x2);
        if (slot[s] >= 0) {
          int ids[8];
          corner_ids(Lv.vals, (unsigned int)slot[s], ids);
          const Axis X = axis_weight<POLY>(x0, Lv.res, Lv.dres), Y = axis_weight<POLY>(x1, Lv.res, Lv.dres),
                     Z = axis_weight<POLY>(x2, Lv.res, Lv.dres);
          float wc[8];
          corner_weights(X.t, Y.t, Z.t, wc);
          float dw[8][3];
          corner_weight_grads(X, Y, Z, dw);
#pragma unroll
          for (int cc = 0; cc < 8; ++cc) {
            const float4* rp = reinterpret_cast<const float4*>(Lv.feat + (long long)ids[cc] * F);
            const float4 r0 = rp[0], r1 = rp[1];
            const float rr[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
#pragma unroll
            for (int q = 0; q < F; ++q) {
              f[q] = fmaf(wc[cc], rr[q], f[q]);
              A[q][0] = fmaf(dw[cc][0], rr[q], A[q][0]);
              A[q][1] = fmaf(dw[cc][1], rr[q], A[q][1]);
              A[q][2] = fmaf(dw[cc][2], rr[q], A[q][2]);
            }
          }
        }
      }
      // ---- decoder forward for the ReLU masks, k_sem_step's way: ROLLED loops over the weight rows (scalar loads), the lane's
      //      vectors in registers, what a rolled loop produces or consumes element by element in the lane's own LDS row
      const int rows = opaque(H);
      unsigned m1 = 0u;
NRM_ROW_LOOP(4)
      for (int k = 0; k < rows; ++k) {
        float z = w.B1[k];
#pragma unroll
        for (int q = 0; q < F; ++q) z = fmaf(w.W1[k * F + q], f[q], z);
        m1 |= (z > 0.f ? 1u : 0u) << k;
        row[k] = fmaxf(z, 0.f);
      }
      wave_lds_fence();
      float v1[H];
      {
        float h1[H];
#pragma unroll
        for (int k = 0; k < H; ++k) h1[k] = row[k], v1[k] = 0.f;
        wave_lds_fence();
        // h2's masks, and v1 = W2^T (m2 .* w3) on the same pass over W2
NRM_ROW_LOOP(2)
        for (int jx = 0; jx < rows; ++jx) {
          float z = w.B2[jx];
#pragma unroll
          for (int k = 0; k < H; ++k) z = fmaf(w.W2[jx * H + k], h1[k], z);
          const bool on = z > 0.f;
          m2 |= (on ? 1u : 0u) << jx;
          const float v2 = on ? w.W3[jx] : 0.f;
#pragma unroll
          for (int k = 0; k < H; ++k) v1[k] = fmaf(w.W2[jx * H + k], v2, v1[k]);
        }
      }
      // v1 = m1 .* (...), left at row[0,32): where the first contraction phase reads it
#pragma unroll
      for (int k = 0; k < H; ++k) row[k] = ((m1 >> k) & 1u) ? v1[k] : 0.f;
      wave_lds_fence();
NRM_ROW_LOOP(8)
      for (int k = 0; k < rows; ++k) {
        const float vk = row[k];
#pragma unroll
        for (int q = 0; q < F; ++q) J[q] = fmaf(w.W1[k * F + q], vk, J[q]);
      }
      float g[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < F; ++q) {
        g[0] = fmaf(J[q], A[q][0], g[0]);
        g[1] = fmaf(J[q], A[q][1], g[1]);
        g[2] = fmaf(J[q], A[q][2], g[2]);
      }
      // ---- the term: loss and q = dL/dg
      accloss += (double)P::term(g, ln, lane, scale, qv);
      live = qv[0] != 0.f || qv[1] != 0.f || qv[2] != 0.f;
      if (wgrad && live) {
        // ---- second-order pieces: r = A q, a1 = m1 .* (W1 r), a2 = m2 .* (W2 a1); the lane's row for the first contraction
        //      phase: [0,32) v1 | [32,40) r | [40,72) a2 (a1 passes through [40,72) into registers, where it waits for the second)
        float rq[F];
#pragma unroll
        for (int q = 0; q < F; ++q) rq[q] = A[q][0] * qv[0] + A[q][1] * qv[1] + A[q][2] * qv[2];
#pragma unroll
        for (int q = 0; q < F; ++q) row[32 + q] = rq[q];
NRM_ROW_LOOP(4)
        for (int k = 0; k < rows; ++k) {
          float tt = 0.f;
#pragma unroll
          for (int q = 0; q < F; ++q) tt = fmaf(w.W1[k * F + q], rq[q], tt);
          row[40 + k] = ((m1 >> k) & 1u) ? tt : 0.f;
        }
        wave_lds_fence();
#pragma unroll
        for (int k = 0; k < H; ++k) a1[k] = row[40 + k];
        wave_lds_fence();
NRM_ROW_LOOP(2)
        for (int jx = 0; jx < rows; ++jx) {
          float tt = 0.f;
#pragma unroll
          for (int k = 0; k < H; ++k) tt = fmaf(w.W2[jx * H + k], a1[k], tt);
          row[40 + jx] = ((m2 >> jx) & 1u) ? tt : 0.f;
        }
      }
    }
    if (wgrad && !live) {  // a lane that sits out (or used its row as scratch above) contributes zeros to the contractions
#pragma unroll
      for (int k = 0; k < 72; ++k) row[k] = 0.f;
    }
    if (!__any(live)) continue;  // no point of the tile has a gradient (wave-uniform)
    if (wgrad) {  // every lane of the wave from here on: each owns a few entries of the three sums
      wave_lds_fence();
      float dummy = 0.f;
      contract64r<4>(st, jj, 32 + hi * 4, accW1, dummy, false);  // dW1 += v1 (x) r
#pragma clang loop vectorize(disable) interleave(disable) unroll_count(4)
      for (int pp = 0; pp < 64; ++pp) accw3 += st[pp * ST + 40 + jj];  // dw3 += a2
      wave_lds_fence();
      const unsigned m2l = live ? m2 : 0u;
#pragma unroll
      for (int jx = 0; jx < H; ++jx) row[jx] = ((m2l >> jx) & 1u) ? w.W3[jx] : 0.f;
#pragma unroll
      for (int k = 0; k < H; ++k) row[32 + k] = a1[k];
      wave_lds_fence();
      contract64r<16>(st, jj, 32 + hi * 16, accW2, dummy, false);  // dW2 += v2 (x) a1
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
      const bool hit = live && slot[s] >= 0;
      int ids[8];
      corner_ids(Lv.vals, hit ? (unsigned int)slot[s] : 0u, ids);
      if constexpr (P::kFlags) {  // the rows this lane's point adds to are flagged for the active-row Adam (k_mark_touched's store)
        unsigned char* tf = a.touched[s];
        if (tf && hit) {
#pragma unroll
          for (int c = 0; c < 8; ++c) tf[ids[c]] = 1;
        }
      }
      const Axis X = axis_weight<POLY>(x0, Lv.res, Lv.dres), Y = axis_weight<POLY>(x1, Lv.res, Lv.dres),
                 Z = axis_weight<POLY>(x2, Lv.res, Lv.dres);
      float dw[8][3];
      corner_weight_grads(X, Y, Z, dw);
      float csum = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float cq = dw[c][0] * qv[0] + dw[c][1] * qv[1] + dw[c][2] * qv[2];
        csum += cq;
        const int sid = hit ? ids[c] : -1;
#pragma unroll
        for (int G = 0; G < 8; ++G) {
          const int id = __shfl(sid, G * 8 + sub, 64);
          const float cf = __shfl(cq, G * 8 + sub, 64);
          if (id >= 0) atomic_add_f32(Lv.grad + (long long)id * F + fi, cf * gval[G]);
        }
      }
      // a miss: all eight corners address the trash row, which receives sum_c (dw_c . q) J — one atomic per wave and feature
      const bool miss = live && slot[s] < 0;
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
  accloss = wave_sum_d(accloss);
  __syncthreads();
  constexpr int NV = 21;
  float vals[NV];
#pragma unroll
  for (int q = 0; q < 16; ++q) vals[q] = accW2[q];
#pragma unroll
  for (int q = 0; q < 4; ++q) vals[16 + q] = accW1[q];
  vals[20] = accw3;
  if (wgrad) {
#pragma unroll
    for (int v = 0; v < NV; ++v) s_stage[(wv * NV + v) * 64 + lane] = vals[v];
  }
  if (lane == 0) s_loss[wv] = accloss;
  __syncthreads();
  if (wv == 0) {
    if (wgrad) {
      float* mine = reinterpret_cast<float*>(a.ws + kPartOff) + (size_t)blockIdx.x * PW;
#pragma unroll
      for (int ww = 1; ww < kWaves; ++ww) {
#pragma unroll
        for (int v = 0; v < NV; ++v) vals[v] += s_stage[(ww * NV + v) * 64 + lane];
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) mine[P_W2 + jj * H + hi * 16 + q] = vals[q];
#pragma unroll
      for (int q = 0; q < 4; ++q) mine[P_W1 + jj * F + hi * 4 + q] = vals[16 + q];
      if (hi == 0) mine[P_W3 + jj] = vals[20];
    }
    if (lane == 0) {
      double s = s_loss[0];
#pragma unroll
      for (int ww = 1; ww < kWaves; ++ww) s += s_loss[ww];
      reinterpret_cast<double*>(a.ws + kLossOff)[blockIdx.x] = s;
    }
  }
  if (gterm_grid_sum(a, wgrad, ns, s_flag) && threadIdx.x == 0) P::finish(a, cx);
}

// Launch shape: k_sem_step's — four waves per workgroup, a tile each, at most kMaxBlocks workgroups with a grid stride past
// 64 K lanes; it depends on the tile count alone, so equal batches sum in equal order.
inline unsigned gterm_blocks(long long tiles) {
  const long long b = (tiles + kWaves - 1) / kWaves;
  return (unsigned)(b > kMaxBlocks ? kMaxBlocks : b);
}

}  // namespace
}  // namespace shine
