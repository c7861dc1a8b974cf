// shine_mlp.hip — Tier A: Decoder.sdf (model/decoder.py:49-63) as a twice-differentiable op.
//
// The reference's decoder is three nn.Linear + ReLU; autograd differentiates it once for cur_loss.backward()
// (shine_batch.py:208-209) and twice when get_gradient(create_graph=True) feeds the eikonal term
// (utils/tools.py:175-185, shine_batch.py:141-142,182-185).  Here each of the three passes is one launch:
//   forward            pred = w3 . relu(W2 relu(W1 f + b1) + b2) + b3
//   backward           given g = d loss / d pred:  d/df = g J  (J = W1^T (m1 .* W2^T (m2 .* w3))) and the six weight grads
//   backward-backward  given r = d loss / d(d/df):  d/dg = r . J,  dW1 += g v1 (x) r,  dW2 += g v2 (x) a1,  dw3 += g a2
//                      (a1 = m1 .* W1 r,  a2 = m2 .* W2 a1; the ReLU masks are piecewise constant: nothing flows to f)
// lane = point, the weights are wave-uniform scalar loads (constant address space -> SGPR operands), activations are
// recomputed from `feat` in every pass (8 floats in, nothing saved between passes); weight grads contract over the
// wave's 64 points through LDS staging rows into lane-owned accumulators that live across the tile loop, summed over the
// workgroup's four waves and flushed once per workgroup with fp32 atomics.
// This tier keeps the reference's drivers unchanged; the benchmarked path is the fused step (shine_step_v3.hip).
// The two backward passes are k_mlp_bwd<MODE> (shine_mlp_body.hpp, shared with shine_time_mlp.hip).
#include "shine_mlp_body.hpp"

namespace shine {

// ---- forward: lane = point, everything in registers (sdf_decode, device.hpp)
__global__ __launch_bounds__(256) void k_mlp_fwd(MlpArgs a) {
  const MlpDev W = mlp_dev(a.mlp);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long long)gridDim.x * 256) {
    const float4* row = reinterpret_cast<const float4*>(a.feat + i * F);
    const float4 r0 = row[0], r1 = row[1];
    const float f[F] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
    a.pred[i] = sdf_decode(W, f, opaque(H));
  }
}

}  // namespace shine

using namespace shine;

extern "C" int shine_mlp_forward(const float* feat, int64_t n, const float* const* mlp, float* pred_out, void* stream) {
  MlpArgs a = {};
  int rc = fill_args(&a, "shine_mlp_forward: null argument", feat, n, mlp, nullptr);
  if (rc != SHINE_OK) return rc;
  if (n > 0 && !pred_out) return set_error(SHINE_E_INVALID, "shine_mlp_forward: null output");
  if (n == 0) return SHINE_OK;
  a.pred = pred_out;
  hipLaunchKernelGGL(k_mlp_fwd, dim3(mlp_grid(n)), dim3(256), 0, (hipStream_t)stream, a);
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}

extern "C" int shine_mlp_backward(const float* feat, const float* grad_pred, int64_t n, const float* const* mlp,
                                  float* grad_feat_out, float* const* grad_mlp, void* stream) {
  MlpArgs a = {};
  int rc = fill_args(&a, "shine_mlp_backward: null argument", feat, n, mlp, grad_mlp);
  if (rc != SHINE_OK) return rc;
  if (n > 0 && !grad_pred) return set_error(SHINE_E_INVALID, "shine_mlp_backward: null grad_pred");
  if (n == 0 || (!grad_feat_out && !grad_mlp)) return SHINE_OK;
  a.g = grad_pred;
  a.grad_feat = grad_feat_out;
  hipLaunchKernelGGL(k_mlp_bwd<1>, dim3(mlp_bwd_grid(n, grad_mlp != nullptr)), dim3(256), 0, (hipStream_t)stream, a);
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}

extern "C" int shine_mlp_backward_backward(const float* feat, const float* grad_pred, const float* gg_feat, int64_t n,
                                           const float* const* mlp, float* grad_gpred_out, float* const* grad_mlp,
                                           void* stream) {
  MlpArgs a = {};
  int rc = fill_args(&a, "shine_mlp_backward_backward: null argument", feat, n, mlp, grad_mlp);
  if (rc != SHINE_OK) return rc;
  if (n > 0 && (!grad_pred || !gg_feat)) return set_error(SHINE_E_INVALID, "shine_mlp_backward_backward: null input");
  if (n == 0 || (!grad_gpred_out && !grad_mlp)) return SHINE_OK;
  a.g = grad_pred;
  a.r = gg_feat;
  a.grad_g = grad_gpred_out;
  hipLaunchKernelGGL(k_mlp_bwd<2>, dim3(mlp_bwd_grid(n, grad_mlp != nullptr)), dim3(256), 0, (hipStream_t)stream, a);
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}
