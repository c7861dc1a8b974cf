// shine_loss_modes.hip — the training objectives the yamls can select besides sdf_bce (Tier A, the strict drop-in):
//
//   shine_sdf_diff_loss    sdf_diff_loss (utils/loss.py:6-14): main_loss_type sdf_l1 / sdf_l2
//   shine_ray_render_loss  batch_ray_rendering_loss (utils/loss.py:82-118): ray_loss with main_loss_type dr / dr_neus
//
// Each is ONE launch that writes the loss and d loss / d (prediction) for an upstream gradient of 1 — what the torch composite
// computes in a dozen small forward launches and more in its backward.  The grid-wide sum is deterministic: every workgroup
// publishes an fp64 partial, the last one to arrive (shine_arrive.hpp) adds them up in a fixed order and resets the counter.
// Repeated calls give the same bits.
#include "shine_arrive.hpp"
#include "shine_internal.hpp"
#include "shine_ray_render.hpp"

// The composite rounds every product and sum on its own; so do these kernels (no a * b + c contracted into one rounding).
// Saturated rays (a probability of exactly 0 or 1) make the autograd form of the gradient a difference of ~1e10-sized terms:
// its result depends on each of those roundings.
#pragma clang fp contract(off)

namespace shine {
namespace {

constexpr int kMaxBlocks = 1024;  // fp64 partials in the workspace; the counter follows them
static_assert(kMaxBlocks * 8 + 8 <= SHINE_LOSS_WORKSPACE_BYTES, "workspace layout");

__device__ __forceinline__ unsigned* ticket_counter(double* ws) { return reinterpret_cast<unsigned*>(ws + kMaxBlocks); }

// sum of `acc` over the grid, times `scale`, into *loss_out.  s_red: NT / 64 + 1 doubles of LDS.  Called by every thread of
// every workgroup (block-uniform control flow).
template <int NT>
__device__ void grid_sum(double acc, double scale, double* ws, float* loss_out, double* s_red) {
  constexpr int NW = NT / 64;
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (gridDim.x == 1) {
    if (threadIdx.x == 0) {
      double t = 0.0;
      for (int k = 0; k < NW; ++k) t += s_red[k];
      *loss_out = (float)(t * scale);
    }
    return;
  }
  unsigned* cnt = ticket_counter(ws);
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int k = 0; k < NW; ++k) t += s_red[k];
    ws[blockIdx.x] = t;
  }
  if (!arrive_last(cnt, gridDim.x, reinterpret_cast<unsigned*>(s_red + NW))) return;
  double v = 0.0;
  for (int k = threadIdx.x; k < (int)gridDim.x; k += NT) v += ws[k];
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int k = 0; k < NW; ++k) t += s_red[k];
    *loss_out = (float)(t * scale);
    __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next call
  }
}

// ---- sdf_diff_loss: diff_m = (pred - label) / scale; loss = sum(w diff_m^2) / N (L2) or sum(w |diff_m|) / N (L1), the
// gradient in the order autograd forms it: ((1/N) w) (2 diff_m) / scale, ((1/N) w) sgn(diff_m) / scale (sgn(0) = 0).
constexpr int kDiffThreads = 256;

template <bool L2>
__global__ __launch_bounds__(kDiffThreads) void k_sdf_diff_loss(const float* __restrict__ pred, const float* __restrict__ label,
                                                                const float* __restrict__ weight, long long n, float scale,
                                                                float inv_n, double dinv_n, float* loss_out,
                                                                float* __restrict__ dpred, double* ws) {
  __shared__ double s_red[kDiffThreads / 64 + 1];
  double acc = 0.0;
  const long long stride = (long long)gridDim.x * kDiffThreads;
  for (long long i = (long long)blockIdx.x * kDiffThreads + threadIdx.x; i < n; i += stride) {
    const float dm = (pred[i] - label[i]) / scale;
    const float w = weight[i];
    float g;
    if (L2) {
      acc += (double)(w * (dm * dm));
      g = ((inv_n * w) * (2.0f * dm)) / scale;
    } else {
      acc += (double)(w * fabsf(dm));
      const float sg = dm > 0.f ? 1.f : (dm < 0.f ? -1.f : 0.f);
      g = ((inv_n * w) * sg) / scale;
    }
    if (dpred) dpred[i] = g;
  }
  grid_sum<kDiffThreads>(acc, dinv_n, ws, loss_out, s_red);
}

// ---- batch_ray_rendering_loss: one lane per ray, 128 rays per chunk staged through LDS (row stride S | 1: the lanes' reads
// of their own rows hit 32 different banks), the row kept in registers of a fully unrolled S_MAX-element network.
constexpr int kRayThreads = 128;

// (the sort key ray_key_gt and the per-sample arithmetic: shine_ray_render.hpp, shared with the ray step)
__device__ __forceinline__ void cmpx(float& xa, float& ya, int& ia, float& xb, float& yb, int& ib, bool up, int S) {
  const bool a_gt = ray_key_gt(xa, ia, xb, ib, S);
  const bool swap = up ? a_gt : !a_gt;
  const float tx = xa, ty = ya;
  const int ti = ia;
  xa = swap ? xb : xa, ya = swap ? yb : ya, ia = swap ? ib : ia;
  xb = swap ? tx : xb, yb = swap ? ty : yb, ib = swap ? ti : ib;
}

template <int SM, bool NEUS>
__global__ __launch_bounds__(kRayThreads) void k_ray_render_loss(const float* __restrict__ x, const float* __restrict__ y,
                                                                  const float* __restrict__ d_meas, long long R, int S,
                                                                  float inv_r, double dinv_r, float* loss_out,
                                                                  float* __restrict__ dy, double* ws) {
  extern __shared__ double s_dyn[];
  double* s_red = s_dyn;  // kRayThreads / 64 + 1 doubles (4 reserved)
  const int stride = S | 1;
  float* sx = reinterpret_cast<float*>(s_dyn + 4);
  float* sy = sx + kRayThreads * stride;
  const int A = NEUS ? S - 1 : S;  // alphas per ray
  double acc = 0.0;
  const long long chunks = (R + kRayThreads - 1) / kRayThreads;
  for (long long ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const long long r0 = ch * kRayThreads;
    const int nr = (int)((R - r0) < kRayThreads ? (R - r0) : kRayThreads);
    const int ne = nr * S;
    const float* xb = x + r0 * S;
    const float* yb = y + r0 * S;
    __syncthreads();  // (the previous chunk's gradient rows have been written out)
    for (int e = threadIdx.x; e < ne; e += kRayThreads) {
      const int rr = e / S, k = e - rr * S;
      sx[rr * stride + k] = xb[e];
      sy[rr * stride + k] = yb[e];
    }
    __syncthreads();
    const int lr = threadIdx.x;
    if (lr < nr) {
      float vx[SM], vy[SM];
      int id[SM];
#pragma unroll
      for (int k = 0; k < SM; ++k) {
        const bool in = k < S;
        vx[k] = in ? sx[lr * stride + k] : 0.f;
        vy[k] = in ? sy[lr * stride + k] : 0.f;
        id[k] = k;
      }
      // bitonic network on (x, column)
#pragma unroll
      for (int kk = 2; kk <= SM; kk <<= 1) {
#pragma unroll
        for (int j = kk >> 1; j > 0; j >>= 1) {
#pragma unroll
          for (int i = 0; i < SM; ++i) {
            const int l = i ^ j;
            if (l > i) cmpx(vx[i], vy[i], id[i], vx[l], vy[l], id[l], (i & kk) == 0, S);
          }
        }
      }
      // forward, in the composite's order: a, o = (1 - a) + 1e-10, c = cumprod(o) (accumulated in fp64 as torch's CPU
      // kernel does), w = (c / o) a, d = sum w x
      float a[SM], o[SM], c[SM];
      double cp = 1.0;
      float d = 0.f;
#pragma unroll
      for (int k = 0; k < SM; ++k) {
        a[k] = 0.f, o[k] = 1.f, c[k] = 1.f;
        if (k < A) {
          if (NEUS) {
            if (k + 1 < SM) a[k] = ray_neus_alpha(vy[k], vy[k + 1]);
          } else {
            a[k] = vy[k];
          }
          ray_forward(a[k], vx[k], cp, o[k], c[k], d);
        }
      }
      const float dm = d_meas[r0 + lr];
      const float err = d - dm;
      acc += (double)fabsf(err);
      // backward for an upstream gradient of 1: mean -> abs -> sum -> w x -> (c / o) a -> cumprod -> (1 - a) + 1e-10
      // [-> clamp -> the neus quotient], walking the samples from the far end (the reversed cumsum of cumprod's backward)
      const float gd = ray_err_grad(err, inv_r);
      float gy[SM];
      double rc = 0.0;
#pragma unroll
      for (int k = SM - 1; k >= 0; --k) {
        gy[k] = 0.f;
        if (k < A) {
          const float ga_t = ray_backward(gd, vx[k], a[k], o[k], c[k], rc, A == 1);
          if (NEUS) {
            if (k + 1 < SM) {
              float gnum;
              ray_neus_backward(vy[k], vy[k + 1], ga_t, gnum, gy[k]);
              gy[k + 1] += gnum;
            }
          } else {
            gy[k] = ga_t;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < SM; ++k)
        if (k < S) sy[lr * stride + (id[k] < S ? id[k] : 0)] = gy[k];  // back to the unsorted columns (gather's backward)
    }
    __syncthreads();
    float* ob = dy + r0 * S;
    for (int e = threadIdx.x; e < ne; e += kRayThreads) {
      const int rr = e / S, k = e - rr * S;
      ob[e] = sy[rr * stride + k];
    }
  }
  grid_sum<kRayThreads>(acc, dinv_r, ws, loss_out, s_red);
}

template <int SM>
void launch_ray(bool neus, unsigned blocks, size_t lds, hipStream_t st, const float* x, const float* y, const float* d_meas,
                long long R, int S, float* loss_out, float* dy, double* ws) {
  const float inv_r = 1.0f / (float)R;
  const double dinv_r = 1.0 / (double)R;
  if (neus)
    hipLaunchKernelGGL((k_ray_render_loss<SM, true>), dim3(blocks), dim3(kRayThreads), lds, st, x, y, d_meas, R, S, inv_r, dinv_r,
                       loss_out, dy, ws);
  else
    hipLaunchKernelGGL((k_ray_render_loss<SM, false>), dim3(blocks), dim3(kRayThreads), lds, st, x, y, d_meas, R, S, inv_r,
                       dinv_r, loss_out, dy, ws);
}

}  // namespace
}  // namespace shine

using namespace shine;

extern "C" int shine_sdf_diff_loss(const float* pred, const float* label, const float* weight, int64_t n, float scale,
                                   int32_t l2_loss, float* loss_out, float* dpred_out, void* workspace, void* stream) {
  if (n < 1 || !pred || !label || !weight || !loss_out || !workspace || !(scale != 0.f) || ((size_t)workspace & 7))
    return set_error(SHINE_E_INVALID, "shine_sdf_diff_loss: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const long long per = 4LL * kDiffThreads;
  const long long blocks = (n + per - 1) / per;
  const unsigned grid = (unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks);
  const float inv_n = 1.0f / (float)n;
  double* ws = (double*)workspace;
  if (l2_loss)
    hipLaunchKernelGGL(k_sdf_diff_loss<true>, dim3(grid), dim3(kDiffThreads), 0, st, pred, label, weight, (long long)n, scale, inv_n,
                       1.0 / (double)n, loss_out, dpred_out, ws);
  else
    hipLaunchKernelGGL(k_sdf_diff_loss<false>, dim3(grid), dim3(kDiffThreads), 0, st, pred, label, weight, (long long)n, scale,
                       inv_n, 1.0 / (double)n, loss_out, dpred_out, ws);
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}

extern "C" int shine_ray_render_loss(const float* x, const float* y, const float* d_meas, int64_t rays, int32_t samples,
                                     int32_t neus_on, float* loss_out, float* dy_out, void* workspace, void* stream) {
  if (rays < 1 || samples < 1 || !x || !y || !d_meas || !loss_out || !dy_out || !workspace || ((size_t)workspace & 7))
    return set_error(SHINE_E_INVALID, "shine_ray_render_loss: bad argument");
  if (samples > SHINE_RAY_MAX_SAMPLES)
    return set_error(SHINE_E_INVALID, "shine_ray_render_loss: more than SHINE_RAY_MAX_SAMPLES (32) samples per ray");
  if (rays > (1LL << 40)) return set_error(SHINE_E_INVALID, "shine_ray_render_loss: too many rays");
  hipStream_t st = (hipStream_t)stream;
  const long long chunks = (rays + kRayThreads - 1) / kRayThreads;
  const unsigned grid = (unsigned)(chunks < kMaxBlocks ? chunks : kMaxBlocks);
  const size_t lds = 4 * sizeof(double) + 2 * sizeof(float) * (size_t)kRayThreads * (size_t)(samples | 1);
  const bool neus = neus_on != 0;
  double* ws = (double*)workspace;
  if (samples <= 8) launch_ray<8>(neus, grid, lds, st, x, y, d_meas, rays, samples, loss_out, dy_out, ws);
  else if (samples <= 16) launch_ray<16>(neus, grid, lds, st, x, y, d_meas, rays, samples, loss_out, dy_out, ws);
  else launch_ray<32>(neus, grid, lds, st, x, y, d_meas, rays, samples, loss_out, dy_out, ws);
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}
