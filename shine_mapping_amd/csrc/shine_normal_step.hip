// shine_normal_step.hip — the surface-normal term of a training iteration in ONE launch (the drivers' normal_loss_on branch,
// shine_batch.py:192-197, with the two repairs of DESIGN.md 3.18: keepdim in the normalisation and a zero-gradient guard):
//
//   g_i   = d pred_i / d coord_i                    closed form, k_step_v0's EIK chain (no sigma: the term does not depend on it)
//   gh_i  = g_i / |g_i| if |g_i| > 0 else 0         the guard (the eikonal term's: coef = gn > 0 ? ... : 0)
//   l_i   = |gh_i - n_i|_2
//   normal_loss = 1 / n_surf * sum over weight_i > 0 of l_i
//   grads += weight_n * d normal_loss / d {feature tables, W1, W2, w3}     (nothing reaches a bias)
//
// One wave = one tile of 64 batch rows at a time, lane = row (k_sem_step's launch shape and LDS staging, [64][ST] floats per
// wave); the per-row math is k_step_v0's lane-per-point chain, its loops over weight rows ROLLED with scalar loads as in
// k_sem_step (fully unrolled with the weights in LDS it took 256 VGPRs + 256 AGPRs + 1.2 KB of scratch: DESIGN.md 3.18).
// Rows with weight <= 0 sit out behind the weight test (they read no coordinate and no normal); a tile without a surface row
// is skipped as a whole.  Second-order backward with delta = 0: r = A q, a1 = m1 .* (W1 r), a2 = m2 .* (W2 a1);
// dW1 += v1 (x) r, dW2 += v2 (x) a1, dw3 += a2 by contract64r over the staged tile; feature rows += (dw_c/dx . q) J with the
// lanes transposed to (row, feature) as in k_sem_step — one fp32 atomic instruction covers 8 rows x the 8 features of a corner.
//
// The three weight grads and the loss are summed in a fixed order inside a wave and a workgroup and in two ticket levels
// across workgroups (shine_arrive.hpp), so they are bit-identical from call to call; the workgroup that finishes the sum ADDS
// them to grad_mlp and writes the loss.  The loss is summed in fp64 from the lanes up and divided by n_surf in fp64.
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
static_assert(kWorkspaceEnd == SHINE_NORMAL_WORKSPACE_BYTES, "SHINE_NORMAL_WORKSPACE_BYTES is the partial layout above");
static_assert((kGroups + 1) * sizeof(unsigned) <= kCounterBytes && PW % 4 == 0 && kLossOff % 8 == 0, "layout");
static_assert(kGroup <= 64 && kGroups <= 64, "a run's loss partials are read by one wave, a lane each");

#define NRM_LOOP_STR(x) #x
#define NRM_ROW_LOOP(n) _Pragma(NRM_LOOP_STR(clang loop vectorize(disable) interleave(disable) unroll_count(n)))

struct NormalArgs {
  LevelSet ls;
  const float* coord;   // rows of `cstride` floats, x y z first
  const int* idx;       // [n] gather or null
  const float* weight;  // rows of `wstride` floats, the weight first
  const float* normal;  // [.,3], indexed like coord
  const long long* n_surf;
  long long n;
  int cstride, wstride;
  int n_parts;  // entries of n_surf to add up (>= 1)
  float weight_n;
  const float* mlp[6];
  float* gW1;
  float* gW2;
  float* gw3;
  int want_wgrad;
  float* loss_out;
  unsigned char* ws;
};

// q = d (weight_n * normal_loss) / d g of ONE surface row (scale = weight_n / n_surf) and the row's loss term l; the one place
// the term's definition lives: another loss on g (the consistency term) replaces this function and keeps the chain around it.
__device__ __forceinline__ float normal_q(const float (&g)[3], const float (&nl)[3], float scale, float (&q)[3]) {
  q[0] = q[1] = q[2] = 0.f;
  const float gn = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
  if (!(gn > 0.f)) return sqrtf(nl[0] * nl[0] + nl[1] * nl[1] + nl[2] * nl[2]);  // the guard: gh = 0, no gradient
  const float inv = 1.0f / gn;
  const float gh[3] = {g[0] * inv, g[1] * inv, g[2] * inv};
  const float d[3] = {gh[0] - nl[0], gh[1] - nl[1], gh[2] - nl[2]};
  const float l = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  if (l > 0.f) {
    const float il = 1.0f / l;
    const float u[3] = {d[0] * il, d[1] * il, d[2] * il};
    const float ug = u[0] * gh[0] + u[1] * gh[1] + u[2] * gh[2];
    const float c = scale * inv;
    q[0] = c * (u[0] - ug * gh[0]);
    q[1] = c * (u[1] - ug * gh[1]);
    q[2] = c * (u[2] - ug * gh[2]);
  }
  return l;
}

// The sum over the grid of the workgroups' partials, sem_grid_sum's two ticket levels: the last workgroup of each run of kGroup
// to arrive sums that run in index order, the last run to finish sums the run sums in index order, ADDS them to the three
// tensors and writes the loss.  Called by every thread of every workgroup; whoever sums a partial clears it behind itself and the
// counters are reset, so the whole workspace is zero again when the launch ends.
__device__ __forceinline__ void normal_grid_sum(const NormalArgs& a, bool wgrad, long long ns, unsigned* verdict) {
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

  if (!arrive_last(cnt + 1 + grp, gsz, verdict)) return;
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

  if (!arrive_last(cnt, ngrp, verdict)) return;
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
}

template <int L, bool POLY>
__global__ __launch_bounds__(kThreads) void k_normal_step(const NormalArgs a) {
  __shared__ float s_stage[kWaves * 64 * ST];
  __shared__ double s_loss[kWaves];
  __shared__ unsigned s_flag;
  const MlpDev w = mlp_dev(a.mlp);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float* st = s_stage + wv * 64 * ST;
  float* row = st + lane * ST;
  const int jj = lane & 31, hi = lane >> 5;
  const int sub = lane >> 3, fi = lane & 7;
  const bool wgrad = a.want_wgrad != 0;

  long long ns = 0;
  for (int p = 0; p < a.n_parts; ++p) ns += a.n_surf[p];
  const float scale = ns > 0 ? a.weight_n / (float)ns : 0.f;

  float accW2[16], accW1[4];
  float accw3 = 0.f;
  double accloss = 0.0;
#pragma unroll
  for (int q = 0; q < 16; ++q) accW2[q] = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) accW1[q] = 0.f;

  const long long tiles = (a.n + 63) >> 6;
  for (long long t = (long long)blockIdx.x * kWaves + wv; t < tiles; t += (long long)gridDim.x * kWaves) {
    const long long r = t * 64 + lane;
    long long j = 0;
    bool active = false;
    if (r < a.n) {
      j = a.idx ? (long long)a.idx[r] : r;
      active = a.weight[j * a.wstride] > 0.f;
    }
    if (!__any(active)) continue;  // a tile of free-space rows (wave-uniform)

    float x0 = 0.f, x1 = 0.f, x2 = 0.f;
    float qv[3] = {0.f, 0.f, 0.f};
    float J[F];
#pragma unroll
    for (int q = 0; q < F; ++q) J[q] = 0.f;
    int slot[L];
#pragma unroll
    for (int s = 0; s < L; ++s) slot[s] = -1;
    bool live = false;  // a surface row with a gradient (q != 0)
    unsigned m2 = 0u;
    float a1[H];
#pragma unroll
    for (int k = 0; k < H; ++k) a1[k] = 0.f;

    if (active) {
      const float* c = a.coord + j * a.cstride;
      x0 = c[0], x1 = c[1], x2 = c[2];
      const float nl[3] = {a.normal[3 * j], a.normal[3 * j + 1], a.normal[3 * j + 2]};
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
      accloss += (double)normal_q(g, nl, scale, qv);
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
    if (wgrad && !live) {  // a row that sits out (or used its row as scratch above) contributes zeros to the contractions
#pragma unroll
      for (int k = 0; k < 72; ++k) row[k] = 0.f;
    }
    if (!__any(live)) continue;  // no row of the tile has a gradient (wave-uniform)
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
  normal_grid_sum(a, wgrad, ns, &s_flag);
}

// Launch shape: k_sem_step's — four waves per workgroup, a tile each, at most kMaxBlocks workgroups with a grid stride past
// 64 K rows; it depends on n alone, so equal batches sum in equal order.
template <int L, bool POLY>
void launch_normal_step_p(const NormalArgs& a, hipStream_t st) {
  const long long tiles = (a.n + 63) / 64;
  const long long b = (tiles + kWaves - 1) / kWaves;
  hipLaunchKernelGGL((k_normal_step<L, POLY>), dim3((unsigned)(b > kMaxBlocks ? kMaxBlocks : b)), dim3(kThreads), 0, st, a);
}

template <int L>
void launch_normal_step(const NormalArgs& a, bool poly, hipStream_t st) {
  if (poly) launch_normal_step_p<L, true>(a, st);
  else launch_normal_step_p<L, false>(a, st);
}

}  // namespace
}  // namespace shine

using namespace shine;

extern "C" int shine_normal_train_step(const shine_tables* t, const shine_step_config* cfg, const float* coord,
                                       int32_t coord_stride, const int32_t* idx, const float* weight, int32_t weight_stride,
                                       const float* normal, const int64_t* n_surf, int32_t n_surf_parts, int64_t n,
                                       float weight_n, const float* const* feats, const int64_t* rows,
                                       float* const* grad_feats, const float* const* mlp, float* const* grad_mlp,
                                       float* normal_loss_out, void* workspace, void* stream) {
  if (!t) return set_error(SHINE_E_INVALID, "shine_normal_train_step: null table handle");
  if (!cfg) return set_error(SHINE_E_INVALID, "shine_normal_train_step: null config");
  if (coord_stride != 3 && coord_stride != 8)
    return set_error(SHINE_E_INVALID, "shine_normal_train_step: coord_stride is 3 ([n,3] array) or 8 (32-byte pool records)");
  if (weight_stride != 1 && weight_stride != 8)
    return set_error(SHINE_E_INVALID, "shine_normal_train_step: weight_stride is 1 (an array) or 8 (32-byte pool records)");
  if (n < 0) return set_error(SHINE_E_INVALID, "shine_normal_train_step: n < 0");
  if (n_surf_parts < 0) return set_error(SHINE_E_INVALID, "shine_normal_train_step: n_surf_parts < 0");
  if (!feats || !rows || !mlp || !normal_loss_out || (n > 0 && (!coord || !weight || !normal || !n_surf)))
    return set_error(SHINE_E_INVALID, "shine_normal_train_step: null argument");
  if (!workspace || ((size_t)workspace & 255)) return set_error(SHINE_E_INVALID, "shine_normal_train_step: workspace");
  NormalArgs a = {};
  for (int k = 0; k < 6; ++k) {
    if (!mlp[k]) return set_error(SHINE_E_INVALID, "shine_normal_train_step: null decoder parameter");
    a.mlp[k] = mlp[k];
  }
  if (grad_mlp) {
    for (int k = 0; k < 6; ++k)
      if (!grad_mlp[k]) return set_error(SHINE_E_INVALID, "shine_normal_train_step: null weight-grad tensor");
    a.gW1 = grad_mlp[0], a.gW2 = grad_mlp[2], a.gw3 = grad_mlp[4];  // (the three biases receive nothing)
  }
  if (cfg->n_levels > 4) return set_error(SHINE_E_INVALID, "shine_normal_train_step: more than 4 featured levels");
  int rc = make_level_set(t, cfg, feats, rows, grad_feats, &a.ls);
  if (rc != SHINE_OK) return rc;
  const int L = cfg->n_levels;
  for (int s = 0; s < L; ++s) {
    if (!feats[s]) return set_error(SHINE_E_INVALID, "shine_normal_train_step: null feature level");
    if (rows[s] >= (1ll << 29)) return set_error(SHINE_E_INVALID, "shine_normal_train_step: level exceeds 2^29 rows");
  }
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    SHINE_HIP_CHECK(hipMemsetAsync(normal_loss_out, 0, sizeof(float), st));
    return SHINE_OK;
  }
  a.coord = coord;
  a.idx = idx;
  a.weight = weight;
  a.normal = normal;
  a.n_surf = reinterpret_cast<const long long*>(n_surf);
  a.n_parts = n_surf_parts > 1 ? n_surf_parts : 1;
  a.n = n;
  a.cstride = coord_stride;
  a.wstride = weight_stride;
  a.weight_n = weight_n;
  a.want_wgrad = grad_mlp ? 1 : 0;
  a.loss_out = normal_loss_out;
  a.ws = (unsigned char*)workspace;
  const bool poly = cfg->poly_int_on != 0;
  switch (L) {
    case 1: launch_normal_step<1>(a, poly, st); break;
    case 2: launch_normal_step<2>(a, poly, st); break;
    case 3: launch_normal_step<3>(a, poly, st); break;
    default: launch_normal_step<4>(a, poly, st); break;
  }
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}
