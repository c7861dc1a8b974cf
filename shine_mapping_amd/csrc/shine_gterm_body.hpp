// shine_gterm_body.hpp — the ONE chain of the training terms that are a loss on g = d pred / d coord (the surface-normal term,
// shine_normal_step.hip; the gradient-consistency term, shine_consistency_step.hip): the closed-form g of a lane's point, the
// term's q = dL/dg, and the second-order backward of that loss into the feature tables and W1, W2, w3.
//
// One wave = one tile of 64 lanes at a time, lane = point (a term step's launch shape, shine_term_dev.hpp, and the LDS staging
// of the lane-per-point kernels, [64][ST] floats per wave); the per-point math is k_step_v0's lane-per-point chain, its loops
// over weight rows ROLLED with scalar loads (fully unrolled with the weights in LDS it took 256 VGPRs + 256 AGPRs + 1.2 KB of
// scratch: DESIGN.md 3.18).  Second-order backward with delta = 0: r = A q, a1 = m1 .* (W1 r), a2 = m2 .* (W2 a1);
// dW1 += v1 (x) r, dW2 += v2 (x) a1, dw3 += a2 by contract64r over the staged tile; feature rows += (dw_c/dx . q) J with the
// lanes transposed to (row, feature) — one fp32 atomic instruction covers 8 rows x the 8 features of a corner.
//
// The three weight grads and the loss are summed in a fixed order inside a wave and a workgroup and in two ticket levels across
// workgroups (grid_sum_two_level, shine_term_dev.hpp), so they are bit-identical from call to call; the workgroup that finishes
// the sum ADDS them to grad_mlp, writes the loss and leaves the workspace all zero.  The loss is summed in fp64 from the lanes up
// and divided by the term's count in fp64.
//
// Of the shared tail (shine_term_dev.hpp) this body takes the launch shape and the grid sum.  It keeps its own lines for the
// level gather (a helper: 12 to 24 more VGPRs), for the scatter (scatter_corner_rows: k_normal_step<2, false> spills 75 SGPRs, not
// 74) and for the workgroup's partial (tile_partial: k_consistency_step<1, *> spills 2 more SGPRs).
//
// A kernel instantiates gterm_step<L, POLY, P> with a POLICY P that says what a lane's point is, what the term is and what it
// is divided by:
//   P::Args                      the kernel's argument struct; the chain reads ls, mlp, gW1 / gW2 / gw3, want_wgrad, loss_out, ws
//   P::Ctx, P::begin(a)          per-thread launch facts, read once; Ctx has `den` (the term's count, long long) and `scale`
//                                (weight / den, what q is multiplied by)
//   P::tiles(a)                  tiles of 64 lanes
//   P::select(a, cx, t, lane, j, ln)   does the lane have a point in tile t -> bool; j = its row, ln (P::Lane) = what load / term
//                                need
//   P::load(a, j, lane, x0, x1, x2, ln)  the point's coordinates (called by the lanes select() accepted)
//   P::term(g, ln, lane, scale, q)       -> the lane's addend to the loss sum; q = d (weight * loss) / d g of the lane's point
//                                (q == 0: the lane sits out of the backward).  Called by every accepted lane of the wave at once
//   P::kFlags                    the kernel marks a.touched[s][row] = 1 for every corner row a live lane scatters to
//   P::finish(a, cx)             called by thread 0 of the workgroup that finished the grid sum, after the loss is written
#pragma once
#include "shine_term_dev.hpp"

namespace shine {
namespace {

// partial layout (floats): W1 [32][8] | W2 [32][32] | w3 [32]
constexpr int P_W1 = 0, P_W2 = P_W1 + H * F, P_W3 = P_W2 + H * H, PW = P_W3 + H;
// workspace: counters ([0] run-level ticket, [1..kGroups] first-level tickets) | float part[kMaxBlocks][PW] | float run[kGroups][PW]
// | double loss_part[kMaxBlocks] | double loss_run[kGroups]
constexpr size_t kPartOff = kCounterBytes;
constexpr size_t kRunOff = kPartOff + (size_t)kMaxBlocks * PW * sizeof(float);
constexpr size_t kLossOff = kRunOff + (size_t)kGroups * PW * sizeof(float);
constexpr size_t kLossRunOff = kLossOff + (size_t)kMaxBlocks * sizeof(double);
constexpr size_t kWorkspaceEnd = kLossRunOff + (size_t)kGroups * sizeof(double);
static_assert(PW % 4 == 0 && kLossOff % 8 == 0, "layout");

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
      // ---- decoder forward for the ReLU masks: ROLLED loops over the weight rows (scalar loads), the lane's
      //      vectors in registers, what a rolled loop produces or consumes element by element in the lane's own LDS row
      const int rows = opaque(H);
      unsigned m1 = 0u;
TERM_ROW_LOOP(4)
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
TERM_ROW_LOOP(2)
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
TERM_ROW_LOOP(8)
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
TERM_ROW_LOOP(4)
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
TERM_ROW_LOOP(2)
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
  // ADDS the three gradients and writes the loss: the fp64 sum over `den`, 0 without one; a frozen decoder: the loss alone
  const GridSumWs gw = {reinterpret_cast<unsigned*>(a.ws), reinterpret_cast<float*>(a.ws + kPartOff),
                        reinterpret_cast<float*>(a.ws + kRunOff), reinterpret_cast<double*>(a.ws + kLossOff),
                        reinterpret_cast<double*>(a.ws + kLossRunOff)};
  const bool last = grid_sum_two_level<PW, PW / 4, true, 1>(
      gw, wgrad, s_flag,
      [&](int k, float4 s) {
        float* dst = k < P_W2 ? a.gW1 + (k - P_W1) : k < P_W3 ? a.gW2 + (k - P_W2) : a.gw3 + (k - P_W3);
        dst[0] += s.x, dst[1] += s.y, dst[2] += s.z, dst[3] += s.w;  // (a caller's grad tensor may be a 4-byte aligned view)
      },
      [&](const double* sums) { a.loss_out[0] = ns > 0 ? (float)(sums[0] / (double)ns) : 0.f; });
  if (last && threadIdx.x == 0) P::finish(a, cx);
}

}  // namespace
}  // namespace shine
