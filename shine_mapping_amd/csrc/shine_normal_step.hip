// shine_normal_step.hip — the surface-normal term of a training iteration in ONE launch (the drivers' normal_loss_on branch,
// shine_batch.py:192-197, with the two repairs of DESIGN.md 3.18: keepdim in the normalisation and a zero-gradient guard):
//
//   g_i   = d pred_i / d coord_i                    closed form, k_step_v0's EIK chain (no sigma: the term does not depend on it)
//   gh_i  = g_i / |g_i| if |g_i| > 0 else 0         the guard (the eikonal term's: coef = gn > 0 ? ... : 0)
//   l_i   = |gh_i - n_i|_2
//   normal_loss = 1 / n_surf * sum over weight_i > 0 of l_i
//   grads += weight_n * d normal_loss / d {feature tables, W1, W2, w3}     (nothing reaches a bias)
//
// One wave = one tile of 64 batch rows at a time, lane = row.  The chain — g, the second-order backward of a loss on g, the
// feature scatter, the deterministic two-level sum of the weight grads and the loss — is shine_gterm_body.hpp's, shared with the
// gradient-consistency term; this file holds the term (normal_q), the policy that feeds the chain and the entry point.
// Rows with weight <= 0 sit out behind the weight test (they read no coordinate and no normal); a tile without a surface row
// is skipped as a whole.  The loss is summed in fp64 from the lanes up and divided by n_surf in fp64.
#include "shine_gterm_body.hpp"
#include "shine_term_host.hpp"

namespace shine {
namespace {

static_assert(kWorkspaceEnd == SHINE_NORMAL_WORKSPACE_BYTES, "SHINE_NORMAL_WORKSPACE_BYTES is the partial layout of shine_gterm_body.hpp");

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
// the term's definition lives (the consistency term, shine_consistency_step.hip, has another here and the same chain around it).
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

// The chain's policy (shine_gterm_body.hpp): a lane = a batch row, rows with weight <= 0 sit out, the count is n_surf.
struct NormalPolicy {
  using Args = NormalArgs;
  static constexpr bool kFlags = false;  // (the fused step's flags cover the same rows)
  struct Ctx {
    long long den;
    float scale;
  };
  struct Lane {
    float nl[3];
  };
  static __device__ __forceinline__ Ctx begin(const Args& a) {
    long long ns = 0;
    for (int p = 0; p < a.n_parts; ++p) ns += a.n_surf[p];
    return {ns, ns > 0 ? a.weight_n / (float)ns : 0.f};
  }
  static __device__ __forceinline__ long long tiles(const Args& a) { return (a.n + 63) >> 6; }
  static __device__ __forceinline__ bool select(const Args& a, const Ctx&, long long t, int lane, long long& j, Lane&) {
    const long long r = t * 64 + lane;
    if (r >= a.n) return false;
    j = a.idx ? (long long)a.idx[r] : r;
    return a.weight[j * a.wstride] > 0.f;
  }
  static __device__ __forceinline__ void load(const Args& a, long long j, int, float& x0, float& x1, float& x2, Lane& ln) {
    const float* c = a.coord + j * a.cstride;
    x0 = c[0], x1 = c[1], x2 = c[2];
    ln.nl[0] = a.normal[3 * j], ln.nl[1] = a.normal[3 * j + 1], ln.nl[2] = a.normal[3 * j + 2];
  }
  static __device__ __forceinline__ float term(const float (&g)[3], const Lane& ln, int, float scale, float (&q)[3]) {
    return normal_q(g, ln.nl, scale, q);
  }
  static __device__ __forceinline__ void finish(const Args&, const Ctx&) {}
};

template <int L, bool POLY>
__global__ __launch_bounds__(kThreads) void k_normal_step(const NormalArgs a) {
  __shared__ float s_stage[kWaves * 64 * ST];
  __shared__ double s_loss[kWaves];
  __shared__ unsigned s_flag;
  gterm_step<L, POLY, NormalPolicy>(a, s_stage, s_loss, &s_flag);
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
  static const char* const kEntry = "shine_normal_train_step";
  NormalArgs a = {};
  int rc = term_prologue(kEntry, t, cfg, coord_stride, n, feats, rows, normal_loss_out, workspace);
  if (rc == SHINE_OK) rc = term_decoder(kEntry, mlp, grad_mlp, &a);
  if (rc != SHINE_OK) return rc;
  if (weight_stride != 1 && weight_stride != 8)
    return term_refuse(kEntry, "weight_stride is 1 (an array) or 8 (32-byte pool records)");
  if (n_surf_parts < 0) return term_refuse(kEntry, "n_surf_parts < 0");
  if (n > 0 && (!coord || !weight || !normal || !n_surf)) return term_refuse(kEntry, "null argument");
  rc = term_levels(kEntry, t, cfg, feats, rows, grad_feats, &a.ls);
  if (rc != SHINE_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) return term_empty(normal_loss_out, st);
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
  a.loss_out = normal_loss_out;
  a.ws = (unsigned char*)workspace;
  const dim3 grid(term_blocks((n + 63) / 64));
  dispatch_levels_poly(cfg->n_levels, cfg->poly_int_on != 0, [&](auto l, auto p) {
    hipLaunchKernelGGL((k_normal_step<decltype(l)::value, decltype(p)::value>), grid, dim3(kThreads), 0, st, a);
  });
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}
