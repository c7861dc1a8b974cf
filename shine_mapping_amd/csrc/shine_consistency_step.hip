// shine_consistency_step.hip — the gradient-consistency term of a training iteration in ONE launch (the drivers'
// consistency_loss_on branch, shine_batch.py:149-158,187-190 / shine_incre.py:137-146,167-170, with the zero-gradient guard of
// DESIGN.md 3.19):
//
//   a_k   = coord[near_index[k]],  b_k = fl32(a_k + shift[k])              K pairs; every batch row may be a base point
//   ga, gb = d pred / d coord at a_k, b_k                                   closed form, shine_gterm_body.hpp's chain (no sigma)
//   c_k   = (ga . gb) / (|ga| |gb|) if |ga| > 0 and |gb| > 0 else 0         THE GUARD: such a pair contributes 1, no gradient
//   consistency_loss = 1 / K * sum_k (1 - c_k)
//   grads += weight_c * d consistency_loss / d {feature tables, W1, W2, w3} through BOTH points (nothing reaches a bias)
//
// One wave = one tile of 32 pairs: lanes 0-31 hold the base points, lanes 32-63 their shifted partners.  After g each lane
// fetches its partner's g across the wave halves (lane ^ 32) and evaluates the term for ITS point:
// q = -(ph - c gh) / |g| * weight_c / K with gh, ph the unit vectors of its own and its partner's g.  Everything after q is the
// shared chain.  Only lanes 0-31 add 1 - c_k to the loss sum.
//
// Pairs: EXPLICIT (near_index, shift given) or DRAWN by the kernel from (seed, *draw_state) with the project's counter-based
// generator (splitmix64 finaliser of (seed, stream, counter), shine_sampler_dev.hpp): stream = *draw_state, counter = 4 k + j;
// j = 0: the index = (top 32 bits * n) >> 32, no float involved; j = 1..3: shift_j = fmaf(2 u, s, -s) with the 24-bit u.  Every
// workgroup reads *draw_state before it arrives; the workgroup that finishes the grid sum increments it, so a replayed graph draws
// fresh pairs each iteration with no host involvement.
//
// TOUCHED-ROW FLAGS: the shifted points reach corner rows the batch's own points did not; with the exact active-row Adam the
// tail neither steps nor clears a row whose flag is 0 (shine_finish.hip), so every live lane flags the rows it scatters to.
#include "shine_gterm_body.hpp"
#include "shine_term_host.hpp"

namespace shine {
namespace {

static_assert(kWorkspaceEnd == SHINE_CONSISTENCY_WORKSPACE_BYTES,
              "SHINE_CONSISTENCY_WORKSPACE_BYTES is the partial layout of shine_gterm_body.hpp");

struct ConsistencyArgs {
  LevelSet ls;
  const float* coord;  // rows of `cstride` floats, x y z first
  const int* idx;      // [n] gather or null
  const int* near_index;  // [n_pairs] or null (drawn)
  const float* shift;     // [n_pairs][3] or null (drawn)
  unsigned long long* draw_state;  // drawn pairs: the stream id, advanced by the launch; null: explicit pairs
  unsigned long long seed;
  int* near_index_out;  // optional: what was used
  float* shift_out;
  long long n;        // batch rows
  long long n_pairs;  // K > 0
  int cstride;
  float shift_scale;
  float weight_c;
  const float* mlp[6];
  float* gW1;
  float* gW2;
  float* gw3;
  int want_wgrad;
  float* loss_out;
  unsigned char* touched[4];
  unsigned char* ws;
};

// draw j of pair k: the splitmix64 finaliser of (seed, stream, 4 k + j), exp1v's mixing (shine_sampler_dev.hpp)
__device__ __forceinline__ unsigned long long pair_bits(unsigned long long seed, unsigned long long stream, unsigned long long k,
                                                        unsigned j) {
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (stream * 0x100000001B3ull + (4ull * k + j) + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// The term of ONE point of a pair: g its own gradient, p its partner's.  -> c_k (0 behind the guard), q = d (weight_c *
// consistency_loss) / d g with scale = weight_c / K.  Symmetric in (g, p), so both lanes of a pair see the same c_k bits.
__device__ __forceinline__ float consistency_q(const float (&g)[3], const float (&p)[3], float scale, float (&q)[3]) {
  q[0] = q[1] = q[2] = 0.f;
  const float gn = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
  const float pn = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
  if (!(gn > 0.f) || !(pn > 0.f)) return 0.f;  // the guard: the pair contributes 1, no gradient on either side
  const float ig = 1.0f / gn, ip = 1.0f / pn;
  const float gh[3] = {g[0] * ig, g[1] * ig, g[2] * ig};
  const float ph[3] = {p[0] * ip, p[1] * ip, p[2] * ip};
  const float c = gh[0] * ph[0] + gh[1] * ph[1] + gh[2] * ph[2];
  const float s = -scale * ig;
  q[0] = s * (ph[0] - c * gh[0]);
  q[1] = s * (ph[1] - c * gh[1]);
  q[2] = s * (ph[2] - c * gh[2]);
  return c;
}

struct ConsistencyPolicy {
  using Args = ConsistencyArgs;
  static constexpr bool kFlags = true;
  struct Ctx {
    long long den;
    float scale;
    unsigned long long stream;
  };
  struct Lane {
    float sh[3];  // the pair's shift (read by both halves; added by the upper one)
  };
  static __device__ __forceinline__ Ctx begin(const Args& a) {
    return {a.n_pairs, a.weight_c / (float)a.n_pairs, a.draw_state ? a.draw_state[0] : 0ull};
  }
  static __device__ __forceinline__ long long tiles(const Args& a) { return (a.n_pairs + 31) >> 5; }
  static __device__ __forceinline__ bool select(const Args& a, const Ctx& cx, long long t, int lane, long long& j, Lane& ln) {
    const long long k = t * 32 + (lane & 31);
    ln.sh[0] = ln.sh[1] = ln.sh[2] = 0.f;
    if (k >= a.n_pairs) return false;
    long long row;
    if (a.near_index) {
      row = (long long)a.near_index[k];
      ln.sh[0] = a.shift[3 * k], ln.sh[1] = a.shift[3 * k + 1], ln.sh[2] = a.shift[3 * k + 2];
    } else {
      const unsigned long long top = pair_bits(a.seed, cx.stream, (unsigned long long)k, 0u) >> 32;
      row = (long long)((top * (unsigned long long)a.n) >> 32);  // (n < 2^31: the product fits)
      const float s = a.shift_scale;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const float u = (float)(unsigned int)(pair_bits(a.seed, cx.stream, (unsigned long long)k, 1u + d) >> 40) * (1.0f / 16777216.0f);
        ln.sh[d] = fmaf(2.0f * u, s, -s);
      }
    }
    if ((unsigned long long)row >= (unsigned long long)a.n) return false;  // (the caller's precondition; such a pair is left out)
    if (lane < 32) {
      if (a.near_index_out) a.near_index_out[k] = (int)row;
      if (a.shift_out) a.shift_out[3 * k] = ln.sh[0], a.shift_out[3 * k + 1] = ln.sh[1], a.shift_out[3 * k + 2] = ln.sh[2];
    }
    j = a.idx ? (long long)a.idx[row] : row;
    return true;
  }
  static __device__ __forceinline__ void load(const Args& a, long long j, int lane, float& x0, float& x1, float& x2, Lane& ln) {
    const float* c = a.coord + j * a.cstride;
    x0 = c[0], x1 = c[1], x2 = c[2];
    if (lane >= 32) x0 = x0 + ln.sh[0], x1 = x1 + ln.sh[1], x2 = x2 + ln.sh[2];  // b_k = fl32(a_k + shift_k)
  }
  // (called by both lanes of a pair at once: a pair is in the launch with both points or with neither)
  static __device__ __forceinline__ float term(const float (&g)[3], const Lane&, int lane, float scale, float (&q)[3]) {
    const float p[3] = {__shfl(g[0], lane ^ 32, 64), __shfl(g[1], lane ^ 32, 64), __shfl(g[2], lane ^ 32, 64)};
    const float c = consistency_q(g, p, scale, q);
    return lane < 32 ? 1.0f - c : 0.f;
  }
  static __device__ __forceinline__ void finish(const Args& a, const Ctx& cx) {
    if (a.draw_state) a.draw_state[0] = cx.stream + 1;  // (one lane's vector store; every workgroup has read it: all have arrived)
  }
};

template <int L, bool POLY>
__global__ __launch_bounds__(kThreads) void k_consistency_step(const ConsistencyArgs a) {
  __shared__ float s_stage[kWaves * 64 * ST];
  __shared__ double s_loss[kWaves];
  __shared__ unsigned s_flag;
  gterm_step<L, POLY, ConsistencyPolicy>(a, s_stage, s_loss, &s_flag);
}

}  // namespace
}  // namespace shine

using namespace shine;

extern "C" int shine_consistency_train_step(const shine_tables* t, const shine_step_config* cfg, const float* coord,
                                            int32_t coord_stride, const int32_t* idx, int64_t n, const int32_t* near_index,
                                            const float* shift, int64_t n_pairs, float shift_scale, uint64_t seed,
                                            uint64_t* draw_state, int32_t* near_index_out, float* shift_out, float weight_c,
                                            const float* const* feats, const int64_t* rows, float* const* grad_feats,
                                            const float* const* mlp, float* const* grad_mlp, unsigned char* const* touched,
                                            float* consistency_loss_out, void* workspace, void* stream) {
  static const char* const kEntry = "shine_consistency_train_step";
  ConsistencyArgs a = {};
  int rc = term_prologue(kEntry, t, cfg, coord_stride, n, feats, rows, consistency_loss_out, workspace);
  if (rc == SHINE_OK) rc = term_decoder(kEntry, mlp, grad_mlp, &a);
  if (rc != SHINE_OK) return rc;
  if (n >= (1ll << 31)) return term_refuse(kEntry, "n exceeds 2^31 - 1 rows");
  if (n_pairs < 0) return term_refuse(kEntry, "n_pairs < 0");
  if ((near_index != nullptr) != (shift != nullptr))
    return term_refuse(kEntry, "near_index and shift come together (both, or neither: drawn pairs)");
  if (!near_index && !draw_state) return term_refuse(kEntry, "drawn pairs need draw_state");
  if (n_pairs > 0 && n == 0) return term_refuse(kEntry, "n_pairs > 0 with n == 0");
  if (n_pairs > 0 && !coord) return term_refuse(kEntry, "null argument");
  rc = term_levels(kEntry, t, cfg, feats, rows, grad_feats, &a.ls);
  if (rc != SHINE_OK) return rc;
  for (int s = 0; s < cfg->n_levels; ++s) a.touched[s] = touched ? touched[s] : nullptr;
  hipStream_t st = (hipStream_t)stream;
  if (n_pairs == 0) return term_empty(consistency_loss_out, st);
  a.coord = coord;
  a.idx = idx;
  a.near_index = near_index;
  a.shift = shift;
  a.draw_state = near_index ? nullptr : reinterpret_cast<unsigned long long*>(draw_state);
  a.seed = seed;
  a.near_index_out = near_index_out;
  a.shift_out = shift_out;
  a.n = n;
  a.n_pairs = n_pairs;
  a.cstride = coord_stride;
  a.shift_scale = shift_scale;
  a.weight_c = weight_c;
  a.loss_out = consistency_loss_out;
  a.ws = (unsigned char*)workspace;
  const dim3 grid(term_blocks((n_pairs + 31) / 32));
  dispatch_levels_poly(cfg->n_levels, cfg->poly_int_on != 0, [&](auto l, auto p) {
    hipLaunchKernelGGL((k_consistency_step<decltype(l)::value, decltype(p)::value>), grid, dim3(kThreads), 0, st, a);
  });
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}
