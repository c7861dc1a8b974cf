// shine_time_mlp.hip — Tier A: Decoder.time_conditionded_sdf (model/decoder.py:65-81) as a twice-differentiable op.
//
// The reference concatenates the point's time stamp to its feature (shine_batch.py:127-130) and runs the 9 -> 32 -> 32 -> 1
// head.  With W1 = [W1f | w_t] the first layer is W1f f + (b1 + w_t ts): the time input is a per-point shift of the first bias.
// So the three passes are shine_mlp.hip's with one scalar per point:
//   forward            pred = w3 . relu(W2 relu(W1f f + w_t ts + b1) + b2) + b3
//   backward           given g: d/df = g W1f^T (m1 .* W2^T (m2 .* w3)) [n][8], the six weight grads, dW1[:,8] += sum_i ts_i d1_i
//   backward-backward  given r = d loss / d(d/df): d/dg = r . J, dW1f += g v1 (x) r, dW2 += g v2 (x) a1, dw3 += g a2; nothing to
//                      dW1[:,8] or the biases (J depends on w_t and ts through the piecewise-constant ReLU masks only)
// ts gets no gradient.  W1 is nn.Linear(9, 32).weight read in place: [32][9], rows not 16-byte aligned, scalar loads only.
// The two backward passes are k_mlp_bwd<MODE, true> (shine_mlp_body.hpp).
#include "shine_mlp_body.hpp"

namespace shine {

// ---- forward: lane = point, everything in registers; sdf_decode (device.hpp) with the 9-wide first layer
__global__ __launch_bounds__(256) void k_time_mlp_fwd(TimeMlpArgs a) {
  const MlpDev w = mlp_dev(a.mlp);
  const int rows = opaque(H);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long long)gridDim.x * 256) {
    const float4* row = reinterpret_cast<const float4*>(a.feat + i * F);
    const float4 r0 = row[0], r1 = row[1];
    const float f[F] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
    const float ts = a.ts[i];
    float h1[H];
    {
      cfloat *const W1i = relaunder(w.W1), *const B1i = relaunder(w.B1);  // keep the loads inside this point's iteration
#pragma unroll
      for (int j = 0; j < H; ++j) {
        float z = fmaf(W1i[j * (F + 1) + F], ts, B1i[j]);
#pragma unroll
        for (int q = 0; q < F; ++q) z = fmaf(W1i[j * (F + 1) + q], f[q], z);
        h1[j] = fmaxf(z, 0.f);
      }
    }
    float y = w.B3[0];
#pragma clang loop vectorize(disable) interleave(disable) unroll_count(2)
    for (int j = 0; j < rows; ++j) {
      float z = w.B2[j];
#pragma unroll
      for (int k = 0; k < H; ++k) z = fmaf(w.W2[j * H + k], h1[k], z);
      y = fmaf(w.W3[j], fmaxf(z, 0.f), y);
    }
    a.pred[i] = y;
  }
}

static int fill_time_args(TimeMlpArgs* a, const char* what, const float* feat, const float* ts, int64_t n,
                          const float* const* mlp, float* const* grad_mlp) {
  int rc = fill_args(a, what, feat, n, mlp, grad_mlp);
  if (rc != SHINE_OK) return rc;
  if (n > 0 && !ts) return set_error(SHINE_E_INVALID, what);
  a->ts = ts;
  return SHINE_OK;
}

}  // namespace shine

using namespace shine;

extern "C" int shine_time_mlp_forward(const float* feat, const float* ts, int64_t n, const float* const* mlp, float* pred_out,
                                      void* stream) {
  TimeMlpArgs a = {};
  int rc = fill_time_args(&a, "shine_time_mlp_forward: null argument", feat, ts, n, mlp, nullptr);
  if (rc != SHINE_OK) return rc;
  if (n > 0 && !pred_out) return set_error(SHINE_E_INVALID, "shine_time_mlp_forward: null output");
  if (n == 0) return SHINE_OK;
  a.pred = pred_out;
  hipLaunchKernelGGL(k_time_mlp_fwd, dim3(mlp_grid(n)), dim3(256), 0, (hipStream_t)stream, a);
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}

extern "C" int shine_time_mlp_backward(const float* feat, const float* ts, const float* grad_pred, int64_t n,
                                       const float* const* mlp, float* grad_feat_out, float* const* grad_mlp, void* stream) {
  TimeMlpArgs a = {};
  int rc = fill_time_args(&a, "shine_time_mlp_backward: null argument", feat, ts, n, mlp, grad_mlp);
  if (rc != SHINE_OK) return rc;
  if (n > 0 && !grad_pred) return set_error(SHINE_E_INVALID, "shine_time_mlp_backward: null grad_pred");
  if (n == 0 || (!grad_feat_out && !grad_mlp)) return SHINE_OK;
  a.g = grad_pred;
  a.grad_feat = grad_feat_out;
  hipLaunchKernelGGL((k_mlp_bwd<1, true>), dim3(mlp_bwd_grid(n, grad_mlp != nullptr)), dim3(256), 0, (hipStream_t)stream, a);
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}

extern "C" int shine_time_mlp_backward_backward(const float* feat, const float* ts, const float* grad_pred,
                                                const float* gg_feat, int64_t n, const float* const* mlp,
                                                float* grad_gpred_out, float* const* grad_mlp, void* stream) {
  TimeMlpArgs a = {};
  int rc = fill_time_args(&a, "shine_time_mlp_backward_backward: null argument", feat, ts, n, mlp, grad_mlp);
  if (rc != SHINE_OK) return rc;
  if (n > 0 && (!grad_pred || !gg_feat)) return set_error(SHINE_E_INVALID, "shine_time_mlp_backward_backward: null input");
  if (n == 0 || (!grad_gpred_out && !grad_mlp)) return SHINE_OK;
  a.g = grad_pred;
  a.r = gg_feat;
  a.grad_g = grad_gpred_out;
  hipLaunchKernelGGL((k_mlp_bwd<2, true>), dim3(mlp_bwd_grid(n, grad_mlp != nullptr)), dim3(256), 0, (hipStream_t)stream, a);
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}
