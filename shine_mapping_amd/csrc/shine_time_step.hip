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
// The chain below is shine_point_step_body.hpp's (shared with k_ray_step, shine_ray_step.hip); this file holds its TimePolicy — the
// 9-wide head and the BCE's delta — and the entry point.
// One wave = one tile of 64 batch rows at a time, lane = row (a term step's launch shape, shine_term_dev.hpp).  The head has ONE output, so its
// first-order backward is delta = d bce / d pred times the Jacobian chain the eikonal term needs anyway:
//   v2 = m2 .* w3,  v1 = m1 .* (W2^T v2),  J = W1f^T v1 = d pred / d f;   d2 = delta v2,  d1 = delta v1,  d f = delta J
// and with the eikonal term's second-order pieces (q = d loss / d g; r = sigma A q, a1 = m1 .* (W1f r), a2 = m2 .* (W2 a1),
// shine_gterm_body.hpp's chain with delta = 0) every weight gradient is ONE contraction over the tile's 64 staged rows:
//   dW1f += v1 (x) (delta f + r)     dW1[:,8] += v1 . (delta ts)     db1 += v1 . delta
//   dW2  += v2 (x) (delta h1 + a1)   db2 += v2 . delta               dw3 += delta h2 + a2      db3 += delta
// (the second-order part reaches W1f, W2 and w3 only: J depends on w_t, ts and the biases through the ReLU masks alone).
// Feature rows receive (w_c delta + sigma dw_c/dx . q) J through the shared transposed scatter (shine_term_dev.hpp).  The decoder
// layers are rolled loops over weight rows with scalar loads (3.18).
//
// The six weight grads and both loss sums (BCE over the batch, eikonal over the surface rows, fp64 from the lanes up) are
// added in a fixed order inside a wave and a workgroup and in two ticket levels across workgroups (shine_arrive.hpp), so they
// are bit-identical from call to call; the workgroup that finishes the sum ADDS the grads, writes the loss and leaves the
// workspace all zero.
#include "shine_point_step_body.hpp"

namespace shine {
namespace {

using namespace pstep;
constexpr int F9 = F + 1;  // row stride of W1 = [W1f | w_t]

struct TimeStepArgs : PointStepArgs {
  const float* label;  // rows of `lstride` floats
  const float* ts;     // indexed like coord
  int lstride;
  int reduction_sum;
  float inv_n;
};

// The time route's policy of the point-step body (shine_point_step_body.hpp): the 9-wide head, delta from the BCE of the point.
struct TimePolicy {
  using Args = TimeStepArgs;
  static constexpr int W1S = F9;
  static constexpr bool SHIFT = true;
  static constexpr int NL = 2;
  struct Lane {
    float ts, label;
  };
  static __device__ __forceinline__ long long tiles(const Args& a) { return (a.n + 63) >> 6; }
  static __device__ __forceinline__ bool locate(const Args& a, long long t, int lane, long long& r, long long& j, Lane&) {
    r = t * 64 + lane;
    if (r >= a.n) return false;
    j = a.idx ? (long long)a.idx[r] : r;
    return true;
  }
  static __device__ __forceinline__ void load(const Args& a, long long j, Lane& ln) {
    ln.label = a.label[j * a.lstride];
    ln.ts = a.ts[j];
  }
  static __device__ __forceinline__ float shift(const Lane& ln) { return ln.ts; }
  static __device__ __forceinline__ float delta(const Args& a, const Lane& ln, bool valid, int, float y, float*, double* acc) {
    if (!valid) return 0.f;
    const float zt = sigmoidf_acc(ln.label / a.sigma);
    acc[0] += (double)(fmaxf(y, 0.f) - y * zt + log1pf(expf(-fabsf(y))));
    return (sigmoidf_acc(y) - zt) * a.inv_n;
  }
  static __device__ __forceinline__ void store(const Args& a, long long r, float y, float) {
    if (a.pred) a.pred[r] = y;
  }
  // where entry k of the partial layout is added: W1's rows are 9 floats apart and its ninth column is w_t's
  static __device__ __forceinline__ float* grad_dst(const Args& a, int k) {
    if (k < P_WT) return a.gW1 + (k >> 3) * F9 + (k & 7);
    if (k < P_B1) return a.gW1 + (k - P_WT) * F9 + F;
    if (k < P_W2) return a.gb1 + (k - P_B1);
    if (k < P_B2) return a.gW2 + (k - P_W2);
    if (k < P_W3) return a.gb2 + (k - P_B2);
    if (k < P_B3) return a.gw3 + (k - P_W3);
    return k == P_B3 ? a.gb3 : nullptr;
  }
  static __device__ __forceinline__ void finish(const Args& a, const double* sums, long long ns) {
    const double bce = a.reduction_sum ? sums[0] : sums[0] * (double)a.inv_n;
    const double eik = ns > 0 ? sums[1] / (double)ns : 0.0;
    a.loss_out[0] = (float)(bce + (double)a.weight_e * eik);
  }
};

template <int L, bool POLY, bool EIK>
__global__ __launch_bounds__(kThreads) void k_time_step(const TimeStepArgs a) {
  __shared__ float s_stage[kWaves * 64 * TST];
  __shared__ double s_loss[kWaves * TimePolicy::NL];
  __shared__ unsigned s_flag;
  point_step_body<L, POLY, EIK, TimePolicy>(a, s_stage, s_loss, &s_flag);
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
  const PointWork wk = point_layout(workspace, TimePolicy::NL);
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
  const dim3 grid(term_blocks((n + 63) / 64));
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
