// shine_semantic.hip — the semantic head (semantic_on): Decoder(config, is_geo_encoder=False).sem_label_prob / sem_label
// (model/decoder.py:89-101) for the shape of every shipped config, 8 -> 32 -> 32 (ReLU, bias) then nclass_out 32 -> C, C <= 32.
//
//   shine_sem_forward       logp = log_softmax(z) [N, C] and / or label = argmax(logp) [N]          one launch
//   shine_sem_backward      given d loss / d logp: d loss / d feat [N, 8] and the six weight grads   one launch
//   shine_sem_query_labels  coord -> query_feature (as shine_query_points) -> decoder -> label       one launch
//
// lane = point; the weights are wave-uniform scalar loads (constant address space, as in shine_mlp.hip).  Layers are ROLLED loops
// over weight rows; per-row results go through the lane's own LDS row and come back as statically indexed registers.  The log-
// softmax is torch's formulation (z - max - log sum exp(z - max)): no overflow for |z| >> 88.  The label is the argmax of the
// rounded logp with the first index winning ties, exactly torch.argmax(sem_label_prob(f)).
//
// Weight grads are repeat-bit-identical: every wave accumulates its tiles in a fixed order, the four waves of a workgroup are
// summed in a fixed order, and the workgroups' partials meet in the two ticket levels of shine_term_dev.hpp's grid sum.
#include "shine_sem_head.hpp"
#include "shine_term_host.hpp"

namespace shine {
using namespace sem;
namespace {

// ---- forward: one 32-float staging row per lane
__global__ __launch_bounds__(kThreads) void k_sem_fwd(const float* __restrict__ feat, long long n, SemArgsPtrs p, int C,
                                                      float* __restrict__ logp, long long* __restrict__ label) {
  __shared__ float s_row[kThreads * SR];
  const SemW w = sem_weights(p.mlp);
  float* row = s_row + threadIdx.x * SR;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const float4* fr = reinterpret_cast<const float4*>(feat + i * F);
    const float4 r0 = fr[0], r1 = fr[1];
    const float f[F] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
    float h1[H];
    unsigned m1, m2;
    sem_hidden(w, f, row, h1, m1, m2);
    const int best = sem_head(w, row, C);
    if (logp) {
      float* o = logp + i * C;
      for (int c = 0; c < C; ++c) o[c] = row[c];
    }
    if (label) label[i] = best;
  }
}

// ---- backward: one wave = one 64-point tile at a time (staging rows [64][ST] per wave, as shine_mlp.hip's k_mlp_bwd)
__global__ __launch_bounds__(kThreads) void k_sem_bwd(const float* __restrict__ feat, const float* __restrict__ logp,
                                                      const float* __restrict__ dlogp, long long n, SemArgsPtrs p, int C,
                                                      float* __restrict__ dfeat, SemGradPtrs gp, int want_wgrad,
                                                      unsigned char* ws) {
  __shared__ float s_stage[4 * 64 * ST];
  __shared__ unsigned s_flag;
  const SemW w = sem_weights(p.mlp);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* st = s_stage + wv * 64 * ST;
  float* row = st + lane * ST;  // [0,32) left operands, [32,64) right operands
  const int jj = lane & 31, hi = lane >> 5;
  const bool wgrad = want_wgrad != 0;
  const int rows = opaque(H);
  const int nc = opaque(C);

  float accWc[16], accW2[16], accW1[4];
  float accbc = 0.f, accb2 = 0.f, accb1 = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) accWc[q] = 0.f, accW2[q] = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) accW1[q] = 0.f;

  const long long tiles = (n + 63) >> 6;
  for (long long t = (long long)blockIdx.x * kWaves + wv; t < tiles; t += (long long)gridDim.x * kWaves) {
    const long long i = t * 64 + lane;
    const bool valid = i < n;
    float f[F];
#pragma unroll
    for (int q = 0; q < F; ++q) f[q] = 0.f;
    if (valid) {
      const float4* fr = reinterpret_cast<const float4*>(feat + i * F);
      const float4 r0 = fr[0], r1 = fr[1];
      f[0] = r0.x, f[1] = r0.y, f[2] = r0.z, f[3] = r0.w, f[4] = r1.x, f[5] = r1.y, f[6] = r1.z, f[7] = r1.w;
    }
    float h1[H];
    unsigned m1, m2;
    sem_hidden(w, f, row, h1, m1, m2);  // h2 now at row[0..32)
    // dz = dlogp - exp(logp) sum_k dlogp_k  (log_softmax's backward on its saved output); padding lanes / classes: 0
    float sg = 0.f;
    if (valid)
      for (int c = 0; c < nc; ++c) sg += dlogp[i * C + c];
    float h2[H];
#pragma unroll
    for (int k = 0; k < H; ++k) h2[k] = row[k];
#pragma unroll
    for (int k = 0; k < H; ++k) row[32 + k] = h2[k];
    for (int c = 0; c < CM; ++c) {
      float dz = 0.f;
      if (valid && c < nc) dz = dlogp[i * C + c] - expf(logp[i * C + c]) * sg;
      row[c] = dz;
    }
    wave_lds_fence();
    if (wgrad) {  // dWc += dz (x) h2, dbc += dz
      contract64r<16>(st, jj, 32 + hi * 16, accWc, accbc, true);
      wave_lds_fence();
    }
    // dh2 = Wc^T dz; d2 = m2 .* dh2
    float d[H];
#pragma unroll
    for (int k = 0; k < H; ++k) d[k] = 0.f;
TERM_ROW_LOOP(2)
    for (int c = 0; c < nc; ++c) {
      const float dz = row[c];
#pragma unroll
      for (int k = 0; k < H; ++k) d[k] = fmaf(w.WC[c * H + k], dz, d[k]);
    }
    wave_lds_fence();  // (every lane of the wave has read its dz before the rows are overwritten)
#pragma unroll
    for (int k = 0; k < H; ++k) row[k] = ((m2 >> k) & 1u) ? d[k] : 0.f;
#pragma unroll
    for (int k = 0; k < H; ++k) row[32 + k] = h1[k];
    wave_lds_fence();
    if (wgrad) {  // dW2 += d2 (x) h1, db2 += d2
      contract64r<16>(st, jj, 32 + hi * 16, accW2, accb2, true);
      wave_lds_fence();
    }
    // dh1 = W2^T d2; d1 = m1 .* dh1
#pragma unroll
    for (int k = 0; k < H; ++k) d[k] = 0.f;
TERM_ROW_LOOP(2)
    for (int j = 0; j < rows; ++j) {
      const float d2 = row[j];
#pragma unroll
      for (int k = 0; k < H; ++k) d[k] = fmaf(w.W2[j * H + k], d2, d[k]);
    }
    wave_lds_fence();
#pragma unroll
    for (int k = 0; k < H; ++k) row[k] = ((m1 >> k) & 1u) ? d[k] : 0.f;
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
    if (valid && dfeat) {
      float4* o = reinterpret_cast<float4*>(dfeat + i * F);
      o[0] = make_float4(df[0], df[1], df[2], df[3]);
      o[1] = make_float4(df[4], df[5], df[6], df[7]);
    }
    if (wgrad) {  // dW1 += d1 (x) f, db1 += d1
      contract64r<4>(st, jj, 32 + hi * 4, accW1, accb1, true);
    }
    wave_lds_fence();
  }
  if (!wgrad) return;

  // ---- the workgroup's partial: the four waves summed PAIRWISE, (0 + 1) + (2 + 3), through LDS — not tile_partial's index
  //      order, which rounds differently: these grads keep the bits they have always had
  __syncthreads();
  constexpr int NV = 39;
  float vals[NV];
#pragma unroll
  for (int q = 0; q < 16; ++q) vals[q] = accWc[q], vals[16 + q] = accW2[q];
#pragma unroll
  for (int q = 0; q < 4; ++q) vals[32 + q] = accW1[q];
  vals[36] = accbc, vals[37] = accb2, vals[38] = accb1;
#pragma unroll
  for (int v = 0; v < NV; ++v) s_stage[(wv * NV + v) * 64 + lane] = vals[v];
  __syncthreads();
  float* part = reinterpret_cast<float*>(ws + kCounterBytes);
  float* mine = part + (size_t)blockIdx.x * P_N;
  if (wv == 0) {
#pragma unroll
    for (int v = 0; v < NV; ++v)
      vals[v] = (s_stage[v * 64 + lane] + s_stage[(NV + v) * 64 + lane]) +
                (s_stage[(2 * NV + v) * 64 + lane] + s_stage[(3 * NV + v) * 64 + lane]);
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
  sem_grid_sum<P_N, false>(ws, true, gp, C, nullptr, 0.f, &s_flag);  // writes the six gradients
}

// ---- mesh labels: the interpolation of shine_query_points (shine_query.hip), then the head above; nothing but the label leaves
template <int L, bool POLY>
__global__ __launch_bounds__(kThreads) void k_sem_query(LevelSet ls, const float* __restrict__ coord, long long n,
                                                        SemArgsPtrs p, int C, long long* __restrict__ label) {
  __shared__ float s_row[kThreads * SR];
  const SemW w = sem_weights(p.mlp);
  float* row = s_row + threadIdx.x * SR;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const float x0 = coord[3 * i], x1 = coord[3 * i + 1], x2 = coord[3 * i + 2];
    float f[F];
#pragma unroll
    for (int k = 0; k < F; ++k) f[k] = 0.f;
    int slot[L];
#pragma unroll
    for (int s = 0; s < L; ++s) slot[s] = level_slot(ls.lv[s], x0, x1, x2);
#pragma unroll
    for (int s = 0; s < L; ++s) {
      const bool hit = slot[s] >= 0;
      const LevelDev& Lv = ls.lv[s];
      int ids[8];
      corner_ids(Lv.vals, hit ? (unsigned int)slot[s] : 0u, ids);
      const Axis X = axis_weight<POLY>(x0, Lv.res, Lv.dres), Y = axis_weight<POLY>(x1, Lv.res, Lv.dres),
                 Z = axis_weight<POLY>(x2, Lv.res, Lv.dres);
      float wc[8];
      corner_weights(X.t, Y.t, Z.t, wc);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const unsigned int off = (hit ? (unsigned int)ids[c] : 0u) * (unsigned int)F;
        const float4 a = *reinterpret_cast<const float4*>(Lv.feat + off);
        const float4 b = *reinterpret_cast<const float4*>(Lv.feat + off + 4u);
        const float wz = hit ? wc[c] : 0.f;
        f[0] += wz * a.x, f[1] += wz * a.y, f[2] += wz * a.z, f[3] += wz * a.w;
        f[4] += wz * b.x, f[5] += wz * b.y, f[6] += wz * b.z, f[7] += wz * b.w;
      }
    }
    float h1[H];
    unsigned m1, m2;
    sem_hidden(w, f, row, h1, m1, m2);
    label[i] = sem_head(w, row, C);
  }
}

unsigned fwd_grid(long long n) {
  const long long b = (n + kThreads - 1) / kThreads;
  return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

}  // namespace
}  // namespace shine

using namespace shine;

extern "C" int shine_sem_forward(const float* feat, int64_t n, const float* const* mlp, int32_t n_class, float* logp_out,
                                 int64_t* label_out, void* stream) {
  SemArgsPtrs p = {};
  if (n < 0 || (n > 0 && !feat) || (!logp_out && !label_out)) return set_error(SHINE_E_INVALID, "shine_sem_forward: null argument");
  int rc = fill_mlp(&p, mlp, n_class, "shine_sem_forward: decoder parameters / n_class (1..32)");
  if (rc != SHINE_OK) return rc;
  if (n == 0) return SHINE_OK;
  hipLaunchKernelGGL(k_sem_fwd, dim3(fwd_grid(n)), dim3(kThreads), 0, (hipStream_t)stream, feat, (long long)n, p, (int)n_class,
                     logp_out, reinterpret_cast<long long*>(label_out));
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}

extern "C" int shine_sem_backward(const float* feat, const float* logp, const float* grad_logp, int64_t n, const float* const* mlp,
                                  int32_t n_class, float* grad_feat_out, float* const* grad_mlp, void* workspace, void* stream) {
  SemArgsPtrs p = {};
  if (n < 0 || (n > 0 && (!feat || !logp || !grad_logp)))
    return set_error(SHINE_E_INVALID, "shine_sem_backward: null argument");
  int rc = fill_mlp(&p, mlp, n_class, "shine_sem_backward: decoder parameters / n_class (1..32)");
  if (rc != SHINE_OK) return rc;
  SemGradPtrs gp = {};
  if (grad_mlp) {
    if (!workspace || ((size_t)workspace & 255)) return set_error(SHINE_E_INVALID, "shine_sem_backward: workspace");
    for (int k = 0; k < 6; ++k) {
      if (!grad_mlp[k]) return set_error(SHINE_E_INVALID, "shine_sem_backward: null weight-grad output");
      gp.g[k] = grad_mlp[k];
    }
  }
  if (!grad_feat_out && !grad_mlp) return SHINE_OK;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {  // (the weight grads of an empty batch are zeros)
    if (grad_mlp) {
      const size_t sz[6] = {(size_t)H * F, (size_t)H, (size_t)H * H, (size_t)H, (size_t)n_class * H, (size_t)n_class};
      for (int k = 0; k < 6; ++k) SHINE_HIP_CHECK(hipMemsetAsync(grad_mlp[k], 0, sz[k] * sizeof(float), st));
    }
    return SHINE_OK;
  }
  hipLaunchKernelGGL(k_sem_bwd, dim3(term_blocks((n + 63) / 64)), dim3(kThreads), 0, st, feat, logp, grad_logp, (long long)n, p,
                     (int)n_class, grad_feat_out, gp, grad_mlp ? 1 : 0, (unsigned char*)workspace);
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}

extern "C" int shine_sem_query_labels(const shine_tables* t, const shine_step_config* cfg, const float* coord, int64_t n,
                                      const float* const* feats, const int64_t* rows, const float* const* mlp, int32_t n_class,
                                      int64_t* label_out, void* stream) {
  if (n < 0 || !feats || !rows || (n > 0 && (!coord || !label_out)))
    return set_error(SHINE_E_INVALID, "shine_sem_query_labels: null argument");
  SemArgsPtrs p = {};
  int rc = fill_mlp(&p, mlp, n_class, "shine_sem_query_labels: decoder parameters / n_class (1..32)");
  if (rc != SHINE_OK) return rc;
  LevelSet ls = {};
  rc = make_level_set(t, cfg, feats, rows, nullptr, &ls);
  if (rc != SHINE_OK) return rc;
  const int L = cfg->n_levels;
  for (int s = 0; s < L; ++s) {
    if (!feats[s]) return set_error(SHINE_E_INVALID, "shine_sem_query_labels: null feature level");
    if (rows[s] >= (1ll << 29)) return set_error(SHINE_E_INVALID, "shine_sem_query_labels: level exceeds 2^29 rows");
  }
  if (n == 0) return SHINE_OK;
  hipStream_t st = (hipStream_t)stream;
  long long* lab = reinterpret_cast<long long*>(label_out);
  long long blocks = (n + kThreads - 1) / kThreads;
  if (blocks > 256 * 16) blocks = 256 * 16;
  if (!dispatch_levels_poly(L, cfg->poly_int_on != 0, [&](auto l, auto pl) {
        hipLaunchKernelGGL((k_sem_query<decltype(l)::value, decltype(pl)::value>), dim3((unsigned)blocks), dim3(kThreads), 0, st,
                           ls, coord, (long long)n, p, (int)n_class, lab);
      }))
    return set_error(SHINE_E_INVALID, "shine_sem_query_labels: more than 4 featured levels");
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}
