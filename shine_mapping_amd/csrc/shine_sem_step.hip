// shine_sem_step.hip — the semantic term of a training iteration in ONE launch (shine_batch.py:132-133,200-204,
// shine_incre.py:128-129,173-177):
//
//   feature  = query_feature(coord)                 the interpolation of shine_query_points, hash tables probed from the coordinates
//   logp     = sem_label_prob(feature)              the head of shine_semantic.hip (shine_sem_head.hpp), bit for bit its forward
//   sem_loss = mean over rows i % d == 0 of -logp[i, label[i]]
//   grads   += weight_s * d sem_loss / d {feature tables, W1, b1, W2, b2, Wc, bc}
//
// Only the m = ceil(n / d) decimated rows are computed.  One wave = one tile of 64 computed rows at a time, lane = row, exactly
// k_sem_bwd's staging ([64][ST] floats of LDS per wave): forward through the head, dz = weight_s / m * (softmax - onehot), the
// three weight-grad contractions, d feature, then the shared tail of a term step (shine_term_dev.hpp): the transposed
// feature-grad scatter with coefficients w_c, the workgroup's partial and the two-level grid sum.
//
// The six weight grads and the loss are summed in a fixed order inside a wave and a workgroup and in two ticket levels across
// workgroups, so they are bit-identical from call to call; the workgroup that finishes the sum ADDS them to grad_mlp and writes
// the loss.  What bounds the launch at the reference's batch (4096 rows = 64 tiles) is the latency of ONE tile through
// the head and back — the rolled weight-row loops are chains of scalar loads and FMAs — not throughput: 64 waves on 16 CUs.
#include "shine_sem_head.hpp"
#include "shine_term_host.hpp"

namespace shine {
using namespace sem;
namespace {

constexpr int PS = P_N + 4;  // partial stride in floats: the six weight grads, then [P_N] the tile losses
static_assert(kCounterBytes + (size_t)(kMaxBlocks + kGroups) * PS * sizeof(float) <= SHINE_SEM_WORKSPACE_BYTES, "workspace");

struct SemStepArgs {
  LevelSet ls;
  const float* coord;   // rows of `stride` floats, x y z first
  const int* idx;       // [n] gather or null
  const int* labels;    // indexed like coord
  long long n, m;       // batch rows, computed rows ceil(n / d)
  long long d;
  int stride;
  int C;
  float gscale;         // weight_s / m
  float inv_m;
  SemArgsPtrs p;
  SemGradPtrs gp;
  int want_wgrad;
  float* loss_out;
  unsigned char* ws;
};

template <int L, bool POLY>
__global__ __launch_bounds__(kThreads) void k_sem_step(const SemStepArgs a) {
  __shared__ float s_stage[4 * 64 * ST];
  __shared__ unsigned s_flag;
  const SemW w = sem_weights(a.p.mlp);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* st = s_stage + wv * 64 * ST;
  float* row = st + lane * ST;  // [0,32) left operands, [32,64) right operands
  const int jj = lane & 31, hi = lane >> 5;
  const bool wgrad = a.want_wgrad != 0;
  const int rows = opaque(H);
  const int nc = opaque(a.C);

  float accWc[16], accW2[16], accW1[4];
  float accbc = 0.f, accb2 = 0.f, accb1 = 0.f, accloss = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) accWc[q] = 0.f, accW2[q] = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) accW1[q] = 0.f;

  const long long tiles = (a.m + 63) >> 6;
  for (long long t = (long long)blockIdx.x * kWaves + wv; t < tiles; t += (long long)gridDim.x * kWaves) {
    const long long r = t * 64 + lane;  // computed row; batch position r * d
    const bool valid = r < a.m;
    float x0 = 0.f, x1 = 0.f, x2 = 0.f;
    int label = 0;
    if (valid) {
      const long long i = r * a.d;
      const long long j = a.idx ? (long long)a.idx[i] : i;
      const float* c = a.coord + j * a.stride;
      x0 = c[0], x1 = c[1], x2 = c[2];
      label = a.labels[j];
    }
    // ---- query_feature (k_sem_query's interpolation); a padding lane misses everywhere
    float f[F];
#pragma unroll
    for (int k = 0; k < F; ++k) f[k] = 0.f;
    int slot[L];
#pragma unroll
    for (int s = 0; s < L; ++s) slot[s] = valid ? level_slot(a.ls.lv[s], x0, x1, x2) : -1;
#pragma unroll
    for (int s = 0; s < L; ++s) {
      const bool hit = slot[s] >= 0;
      const LevelDev& Lv = a.ls.lv[s];
      int ids[8];
      corner_ids(Lv.vals, hit ? (unsigned int)slot[s] : 0u, ids);
      const Axis X = axis_weight<POLY>(x0, Lv.res, Lv.dres), Y = axis_weight<POLY>(x1, Lv.res, Lv.dres),
                 Z = axis_weight<POLY>(x2, Lv.res, Lv.dres);
      float wc[8];
      corner_weights(X.t, Y.t, Z.t, wc);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const unsigned int off = (hit ? (unsigned int)ids[c] : 0u) * (unsigned int)F;
        const float4 fa = *reinterpret_cast<const float4*>(Lv.feat + off);
        const float4 fb = *reinterpret_cast<const float4*>(Lv.feat + off + 4u);
        const float wz = hit ? wc[c] : 0.f;
        f[0] += wz * fa.x, f[1] += wz * fa.y, f[2] += wz * fa.z, f[3] += wz * fa.w;
        f[4] += wz * fb.x, f[5] += wz * fb.y, f[6] += wz * fb.z, f[7] += wz * fb.w;
      }
    }
    // ---- the head forward: h2 kept in registers, logp left at row[0..C)
    float h1[H];
    unsigned m1, m2;
    sem_hidden(w, f, row, h1, m1, m2);
    float h2[H];
#pragma unroll
    for (int k = 0; k < H; ++k) h2[k] = row[k];
    wave_lds_fence();
    sem_head(w, row, a.C);
    wave_lds_fence();
    // NLLLoss('mean') on the m computed rows: d loss / d logp = -gscale at the label; dz = dlogp - exp(logp) sum_k dlogp_k
    // (in place: every lane rewrites its own row, padding lanes / classes get 0)
    float lp_label = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      float dz = 0.f;
      if (valid && c < nc) {
        const float lp = row[c];
        if (c == label) lp_label = lp;
        dz = (c == label ? -a.gscale : 0.f) + expf(lp) * a.gscale;
      }
      row[c] = dz;
    }
    accloss -= lp_label;
#pragma unroll
    for (int k = 0; k < H; ++k) row[32 + k] = h2[k];
    wave_lds_fence();
    if (wgrad) {  // dWc += dz (x) h2, dbc += dz
      contract64r<16>(st, jj, 32 + hi * 16, accWc, accbc, true);
      wave_lds_fence();
    }
    // dh2 = Wc^T dz; d2 = m2 .* dh2
    float dd[H];
#pragma unroll
    for (int k = 0; k < H; ++k) dd[k] = 0.f;
TERM_ROW_LOOP(2)
    for (int c = 0; c < nc; ++c) {
      const float dz = row[c];
#pragma unroll
      for (int k = 0; k < H; ++k) dd[k] = fmaf(w.WC[c * H + k], dz, dd[k]);
    }
    wave_lds_fence();
#pragma unroll
    for (int k = 0; k < H; ++k) row[k] = ((m2 >> k) & 1u) ? dd[k] : 0.f;
#pragma unroll
    for (int k = 0; k < H; ++k) row[32 + k] = h1[k];
    wave_lds_fence();
    if (wgrad) {  // dW2 += d2 (x) h1, db2 += d2
      contract64r<16>(st, jj, 32 + hi * 16, accW2, accb2, true);
      wave_lds_fence();
    }
    // dh1 = W2^T d2; d1 = m1 .* dh1
#pragma unroll
    for (int k = 0; k < H; ++k) dd[k] = 0.f;
TERM_ROW_LOOP(2)
    for (int j = 0; j < rows; ++j) {
      const float d2 = row[j];
#pragma unroll
      for (int k = 0; k < H; ++k) dd[k] = fmaf(w.W2[j * H + k], d2, dd[k]);
    }
    wave_lds_fence();
#pragma unroll
    for (int k = 0; k < H; ++k) row[k] = ((m1 >> k) & 1u) ? dd[k] : 0.f;
#pragma unroll
    for (int q = 0; q < F; ++q) row[32 + q] = f[q];
    wave_lds_fence();
    // df = W1^T d1
    float df[F];
#pragma unroll
    for (int q = 0; q < F; ++q) df[q] = 0.f;
TERM_ROW_LOOP(8)
    for (int k = 0; k < rows; ++k) {
      const float dk = row[k];
#pragma unroll
      for (int q = 0; q < F; ++q) df[q] = fmaf(w.W1[k * F + q], dk, df[q]);
    }
    if (wgrad) {  // dW1 += d1 (x) f, db1 += d1
      contract64r<4>(st, jj, 32 + hi * 4, accW1, accb1, true);
    }
    wave_lds_fence();
    // ---- feature grads: rows += w_c df
    float gval[8];
    stage_row_grads(st, lane, df, gval);
#pragma unroll
    for (int s = 0; s < L; ++s) {
      const LevelDev& Lv = a.ls.lv[s];
      if (!Lv.grad) continue;  // (wave-uniform)
      const bool hit = slot[s] >= 0;
      int ids[8];
      corner_ids(Lv.vals, hit ? (unsigned int)slot[s] : 0u, ids);
      const Axis X = axis_weight<POLY>(x0, Lv.res, Lv.dres), Y = axis_weight<POLY>(x1, Lv.res, Lv.dres),
                 Z = axis_weight<POLY>(x2, Lv.res, Lv.dres);
      float wc[8];
      corner_weights(X.t, Y.t, Z.t, wc);
      scatter_corner_rows(Lv, ids, hit, valid && !hit, wc, df, gval, lane);
    }
  }

  // ---- the workgroup's partial: its waves summed in index order through LDS
  accloss = wave_sum(accloss);
  __syncthreads();
  constexpr int NV = 40;
  float vals[NV];
#pragma unroll
  for (int q = 0; q < 16; ++q) vals[q] = accWc[q], vals[16 + q] = accW2[q];
#pragma unroll
  for (int q = 0; q < 4; ++q) vals[32 + q] = accW1[q];
  vals[36] = accbc, vals[37] = accb2, vals[38] = accb1, vals[39] = accloss;
  tile_partial<NV>(vals, s_stage, wv, lane);
  if (wv == 0) {
    float* mine = reinterpret_cast<float*>(a.ws + kCounterBytes) + (size_t)blockIdx.x * PS;
    if (wgrad) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        mine[P_WC + jj * H + hi * 16 + q] = vals[q];
        mine[P_W2 + jj * H + hi * 16 + q] = vals[16 + q];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) mine[P_W1 + jj * F + hi * 4 + q] = vals[32 + q];
      if (hi == 0) {
        mine[P_BC + jj] = vals[36];
        mine[P_B2 + jj] = vals[37];
        mine[P_B1 + jj] = vals[38];
      }
    }
    if (lane == 0) mine[P_N] = vals[39];
  }
  // ADDS the six gradients and writes the loss (the three floats behind the loss's slot are summed along and never used); a
  // frozen head: only the loss's column is summed
  sem_grid_sum<PS, true>(a.ws, wgrad, a.gp, a.C, a.loss_out, a.inv_m, &s_flag);
}

}  // namespace
}  // namespace shine

using namespace shine;

extern "C" int shine_sem_train_step(const shine_tables* t, const shine_step_config* cfg, const float* coord, int32_t coord_stride,
                                    const int32_t* idx, const int32_t* labels, int64_t n, int32_t decimation, float weight_s,
                                    const float* const* feats, const int64_t* rows, float* const* grad_feats,
                                    const float* const* mlp, int32_t n_class, float* const* grad_mlp, float* sem_loss_out,
                                    void* workspace, void* stream) {
  static const char* const kEntry = "shine_sem_train_step";
  SemStepArgs a = {};
  int rc = term_prologue(kEntry, t, cfg, coord_stride, n, feats, rows, sem_loss_out, workspace);
  if (rc != SHINE_OK) return rc;
  if (decimation < 1) return term_refuse(kEntry, "decimation < 1");
  rc = fill_mlp(&a.p, mlp, n_class, "shine_sem_train_step: decoder parameters / n_class (1..32)");
  if (rc == SHINE_OK) rc = term_wgrads(kEntry, grad_mlp);
  if (rc != SHINE_OK) return rc;
  for (int k = 0; grad_mlp && k < 6; ++k) a.gp.g[k] = grad_mlp[k];
  if (n > 0 && (!coord || !labels)) return term_refuse(kEntry, "null argument");
  rc = term_levels(kEntry, t, cfg, feats, rows, grad_feats, &a.ls);
  if (rc != SHINE_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) return term_empty(sem_loss_out, st);
  const long long m = (n + decimation - 1) / decimation;
  a.coord = coord;
  a.idx = idx;
  a.labels = labels;
  a.n = n;
  a.m = m;
  a.d = decimation;
  a.stride = coord_stride;
  a.C = n_class;
  a.gscale = weight_s / (float)m;
  a.inv_m = 1.0f / (float)m;
  a.want_wgrad = grad_mlp ? 1 : 0;
  a.loss_out = sem_loss_out;
  a.ws = (unsigned char*)workspace;
  const dim3 grid(term_blocks((m + 63) / 64));
  dispatch_levels_poly(cfg->n_levels, cfg->poly_int_on != 0, [&](auto l, auto p) {
    hipLaunchKernelGGL((k_sem_step<decltype(l)::value, decltype(p)::value>), grid, dim3(kThreads), 0, st, a);
  });
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}
