// shine_ray_step.hip — one training iteration's forward + backward of a map trained by RAY RENDERING in ONE launch (the drivers'
// loop body with config.ray_loss and main_loss_type dr / dr_neus, shine_batch.py:119-130,160-170,172-185,208-209):
//
//   f      = query_feature(coord)                          rows r = ray * S + s of the pool, S samples per ray
//   pred   = w3 . relu(W2 relu(W1 f + b1) + b2) + b3       the plain 8 -> 32 -> 32 -> 1 head
//   y      = sigmoid(pred / sigma_size)                    sigma_size: ONE float in device memory (the optimiser steps it)
//   loss   = batch_ray_rendering_loss(sample_depth, y, ray_depth, neus_on)      mean over rays |sum w x - ray_depth|
//          [+ weight_e * mean over weight > 0 of (1 - |g|)^2,  g = sigma d pred / d coord]
//   grads += d loss / d {feature tables, W1, b1, W2, b2, w3, b3, sigma_size}
//
// The step is the point-step body (shine_point_step_body.hpp) with the plain head and a delta that comes from the render.  A
// tile holds WHOLE rays: (64 / S) * S rows, the remaining lanes are padding that misses everywhere.  After the head's forward
// every lane ranks its sample among its ray's S by (depth, column) — S shuffles, the stable order of torch.sort — and leaves
// (depth, y) at its rank in the ray's LDS rows, columns [32, 38), which are free at that point.  The first lane of each ray then
// walks its S sorted samples forward and backward with the arithmetic of shine_ray_render.hpp (the Tier A loss's, fp64 cumprod
// and reversed cumsum included), and every lane picks d loss / d y up at its rank:
//   delta = dL/dy . y (1 - y) / sigma_size,        d loss / d sigma_size += -dL/dy . y (1 - y) . (pred / sigma_size) / sigma_size
// The render sum (over rays), the eikonal sum (over surface samples) and the sigma_size gradient are the body's three fp64 loss
// sums: fixed order, bit-identical from call to call.  S and dr / dr_neus are runtime values: 16 instantiations (L x POLY x EIK).
#include "shine_point_step_body.hpp"
#include "shine_ray_render.hpp"

namespace shine {
namespace {

using namespace pstep;

struct RayStepArgs : PointStepArgs {
  const float* depth;       // [m * S] sample depths, indexed like coord
  const float* ray_depth;   // [m] measured depths
  const float* sigma_size;  // [1]
  float* sigma_grad;        // [1] or null (a frozen sigma_size)
  float* dpred;             // at the batch position, or null
  long long n_rays;
  int S, rpt;  // samples per ray, rays per tile = 64 / S
  int neus;
  float inv_r;
  double dinv_r;
};

// LDS columns of a sorted sample, in the row of lane (ray's first lane + position): free between the head's forward and the
// contraction phases
constexpr int C_X = 32, C_Y = 33, C_A = 34, C_O = 35, C_C = 36, C_G = 37;

struct RayPolicy {
  using Args = RayStepArgs;
  static constexpr int W1S = F;
  static constexpr bool SHIFT = false;
  static constexpr int NL = 3;  // [2]: d loss / d sigma_size
  struct Lane {
    float x, dm;    // the sample's depth, its ray's measured depth
    int lead, col;  // the ray's first lane, the sample's column (0, 0 on a padding lane)
  };
  static __device__ __forceinline__ long long tiles(const Args& a) { return (a.n_rays + a.rpt - 1) / a.rpt; }
  static __device__ __forceinline__ bool locate(const Args& a, long long t, int lane, long long& r, long long& j, Lane& ln) {
    const int lr = lane / a.S;
    if (lr >= a.rpt) return false;
    ln.col = lane - lr * a.S;
    ln.lead = lane - ln.col;
    const long long ray = t * a.rpt + lr;
    if (ray >= a.n_rays) return false;
    const long long src = a.idx ? (long long)a.idx[ray] : ray;
    r = ray * a.S + ln.col;
    j = src * a.S + ln.col;
    ln.dm = a.ray_depth[src];
    return true;
  }
  static __device__ __forceinline__ void load(const Args& a, long long j, Lane& ln) { ln.x = a.depth[j]; }
  static __device__ __forceinline__ float shift(const Lane&) { return 0.f; }
  static __device__ __forceinline__ float delta(const Args& a, const Lane& ln, bool valid, int, float pred, float* st,
                                                double* acc) {
    const int S = a.S;
    const float ss = a.sigma_size[0];
    const float z = pred / ss;
    const float y = sigmoidf_acc(z);
    // the sample's position in its ray's depth order (ties by column): lanes of one ray are neighbours
    int rank = 0;
    for (int s = 0; s < S; ++s) {
      const float xs = __shfl(ln.x, ln.lead + s, 64);
      rank += ray_key_gt(ln.x, ln.col, xs, s, S) ? 1 : 0;
    }
    float* mine = st + (ln.lead + rank) * TST;
    if (valid) mine[C_X] = ln.x, mine[C_Y] = y, mine[C_G] = 0.f;
    wave_lds_fence();
    if (valid && ln.col == 0) {  // the ray's first lane: the render over its S sorted samples
      float* base = st + ln.lead * TST;
      const bool neus = a.neus != 0;
      const int A = neus ? S - 1 : S;  // alphas per ray
      double cp = 1.0;
      float d = 0.f;
      for (int k = 0; k < A; ++k) {
        float* sr = base + k * TST;
        const float al = neus ? ray_neus_alpha(sr[C_Y], sr[TST + C_Y]) : sr[C_Y];
        float o, c;
        ray_forward(al, sr[C_X], cp, o, c, d);
        sr[C_A] = al, sr[C_O] = o, sr[C_C] = c;
      }
      const float err = d - ln.dm;
      acc[0] += (double)fabsf(err);
      const float gd = ray_err_grad(err, a.inv_r);
      double rc = 0.0;
      for (int k = A - 1; k >= 0; --k) {
        float* sr = base + k * TST;
        const float ga = ray_backward(gd, sr[C_X], sr[C_A], sr[C_O], sr[C_C], rc, A == 1);
        if (neus) {
          float gnum, gown;
          ray_neus_backward(sr[C_Y], sr[TST + C_Y], ga, gnum, gown);
          sr[TST + C_G] += gnum;
          sr[C_G] = gown;
        } else {
          sr[C_G] = ga;
        }
      }
    }
    wave_lds_fence();
    float dl = 0.f;
    if (valid) {
      const float dz = mine[C_G] * ((1.0f - y) * y);  // through the sigmoid
      dl = dz / ss;
      acc[2] += (double)(-dz * (z / ss));
    }
    wave_lds_fence();  // (the contraction phases write these columns next)
    return dl;
  }
  static __device__ __forceinline__ void store(const Args& a, long long r, float y, float dl) {
    if (a.pred) a.pred[r] = y;
    if (a.dpred) a.dpred[r] = dl;
  }
  // where entry k of the partial layout is added: W1 is [32][8], the w_t column of the layout stays empty
  static __device__ __forceinline__ float* grad_dst(const Args& a, int k) {
    if (k < P_WT) return a.gW1 + k;
    if (k < P_B1) return nullptr;
    if (k < P_W2) return a.gb1 + (k - P_B1);
    if (k < P_B2) return a.gW2 + (k - P_W2);
    if (k < P_W3) return a.gb2 + (k - P_B2);
    if (k < P_B3) return a.gw3 + (k - P_W3);
    return k == P_B3 ? a.gb3 : nullptr;
  }
  static __device__ __forceinline__ void finish(const Args& a, const double* sums, long long ns) {
    const double eik = ns > 0 ? sums[1] / (double)ns : 0.0;
    a.loss_out[0] = (float)(sums[0] * a.dinv_r + (double)a.weight_e * eik);
    if (a.sigma_grad) a.sigma_grad[0] += (float)sums[2];
  }
};

template <int L, bool POLY, bool EIK>
__global__ __launch_bounds__(kThreads) void k_ray_step(const RayStepArgs a) {
  __shared__ float s_stage[kWaves * 64 * TST];
  __shared__ double s_loss[kWaves * RayPolicy::NL];
  __shared__ unsigned s_flag;
  point_step_body<L, POLY, EIK, RayPolicy>(a, s_stage, s_loss, &s_flag);
}

// the surface samples of a drawn batch of rays: sum of surf_per_ray[idx[i]] — one workgroup, an exact integer sum
__global__ __launch_bounds__(256) void k_ray_surf_count(const int* __restrict__ idx, const int* __restrict__ surf_per_ray,
                                                        long long n, long long* out) {
  __shared__ long long s_part[4];
  long long c = 0;
  for (long long i = threadIdx.x; i < n; i += 256) c += surf_per_ray[idx ? idx[i] : i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

}  // namespace
}  // namespace shine

using namespace shine;

extern "C" int shine_ray_surf_count(const int32_t* idx, const int32_t* surf_per_ray, int64_t n, int64_t* count_out, void* stream) {
  if (n < 0 || !surf_per_ray || !count_out) return term_refuse("shine_ray_surf_count", "bad argument");
  hipLaunchKernelGGL(k_ray_surf_count, dim3(1), dim3(256), 0, (hipStream_t)stream, idx, surf_per_ray, (long long)n,
                     reinterpret_cast<long long*>(count_out));
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}

extern "C" int shine_ray_step(const shine_tables* t, const shine_step_config* cfg, const float* coord, const int32_t* idx,
                              const float* weight, const float* sample_depth, const float* ray_depth, const float* sigma_size,
                              int32_t samples, int32_t neus_on, const int64_t* n_surf, int32_t n_surf_parts, int64_t n_rays,
                              const float* const* feats, const int64_t* rows, float* const* grad_feats,
                              const float* const* mlp, float* const* grad_mlp, float* sigma_grad, float* pred_out,
                              float* dpred_out, float* loss_out, void* workspace, size_t* workspace_bytes, void* stream) {
  static const char* const kEntry = "shine_ray_step";
  if (!workspace_bytes) return term_refuse(kEntry, "null workspace_bytes");
  const PointWork wk = point_layout(workspace, RayPolicy::NL);
  if (!workspace) {  // the size query (one layout for every batch: the workgroup count is capped)
    *workspace_bytes = wk.bytes;
    return SHINE_OK;
  }
  RayStepArgs a = {};
  int rc = term_prologue(kEntry, t, cfg, 3, n_rays, feats, rows, loss_out, workspace);
  if (rc == SHINE_OK) rc = term_decoder(kEntry, mlp, grad_mlp, &a);
  if (rc != SHINE_OK) return rc;
  SHINE_WORKSPACE_FITS(wk.bytes, workspace, *workspace_bytes, "shine_ray_step");
  if (samples < 1) return term_refuse(kEntry, "samples < 1");
  if (samples > SHINE_RAY_MAX_SAMPLES) return term_refuse(kEntry, "more than SHINE_RAY_MAX_SAMPLES (32) samples per ray");
  if (n_rays >= (1ll << 31) / samples) return term_refuse(kEntry, "n * samples exceeds 2^31 - 1 rows");
  const bool eik = cfg->eikonal_on != 0;
  if (n_surf_parts < 0 || n_surf_parts > 64) return term_refuse(kEntry, "n_surf_parts is 0 .. 64");
  if (n_rays > 0 && (!coord || !sample_depth || !ray_depth || !sigma_size || (eik && (!weight || !n_surf))))
    return term_refuse(kEntry, "null argument");
  rc = term_levels(kEntry, t, cfg, feats, rows, grad_feats, &a.ls);
  if (rc != SHINE_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (n_rays == 0) return term_empty(loss_out, st);
  if (grad_mlp) a.gb1 = grad_mlp[1], a.gb2 = grad_mlp[3], a.gb3 = grad_mlp[5];
  a.coord = coord;
  a.idx = idx;
  a.weight = weight;
  a.wstride = 1;
  a.cstride = 3;
  a.n_surf = reinterpret_cast<const long long*>(n_surf);
  a.n_parts = n_surf_parts > 1 ? n_surf_parts : 1;
  a.n = n_rays * samples;
  a.sigma = cfg->sigma;
  a.weight_e = cfg->weight_e;
  a.pred = pred_out;
  a.loss_out = loss_out;
  a.cnt = wk.cnt, a.part = wk.part, a.run = wk.run, a.lpart = wk.lpart, a.lrun = wk.lrun;
  a.depth = sample_depth;
  a.ray_depth = ray_depth;
  a.sigma_size = sigma_size;
  a.sigma_grad = sigma_grad;
  a.dpred = dpred_out;
  a.n_rays = n_rays;
  a.S = samples;
  a.rpt = 64 / samples;
  a.neus = neus_on != 0;
  a.inv_r = 1.0f / (float)n_rays;
  a.dinv_r = 1.0 / (double)n_rays;
  const dim3 grid(term_blocks((n_rays + a.rpt - 1) / a.rpt));
  dispatch_levels_poly(cfg->n_levels, cfg->poly_int_on != 0, [&](auto l, auto p) {
    constexpr int LL = decltype(l)::value;
    constexpr bool PP = decltype(p)::value;
    if (eik)
      hipLaunchKernelGGL((k_ray_step<LL, PP, true>), grid, dim3(kThreads), 0, st, a);
    else
      hipLaunchKernelGGL((k_ray_step<LL, PP, false>), grid, dim3(kThreads), 0, st, a);
  });
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}
