// shine_sem_head.hpp — the semantic head's device code shared by shine_semantic.hip (forward, backward, mesh labels) and
// shine_sem_step.hip (the training loop's NLL launch): the weight pointers, the two hidden layers, the class layer with its
// log-softmax, the layout of the per-workgroup weight-grad partials and what the grid sum over them (shine_term_dev.hpp) does
// with every summed element (sem_grid_sum).
#pragma once
#include "shine_term_dev.hpp"

namespace shine {
namespace sem {

constexpr int CM = SHINE_SEM_MAX_CLASSES;  // 32
constexpr int SR = 33;                     // forward staging row stride (odd: the lanes' rows hit different banks)
// partial layout (floats): W1 [32][8] | b1 [32] | W2 [32][32] | b2 [32] | Wc [32][32] | bc [32] (Wc / bc padded to 32 classes)
constexpr int P_W1 = 0, P_B1 = P_W1 + H * F, P_W2 = P_B1 + H, P_B2 = P_W2 + H * H, P_WC = P_B2 + H, P_BC = P_WC + CM * H;
constexpr int P_N = P_BC + CM;
static_assert(kCounterBytes + (size_t)(kMaxBlocks + kGroups) * P_N * sizeof(float) <= SHINE_SEM_WORKSPACE_BYTES, "workspace");

struct SemArgsPtrs {
  const float* mlp[6];  // W1 [32][8], b1 [32], W2 [32][32], b2 [32], Wc [C][32], bc [C]
};
struct SemGradPtrs {
  float* g[6];
};

struct SemW {
  cfloat *W1, *B1, *W2, *B2, *WC, *BC;
};

__device__ __forceinline__ SemW sem_weights(const float* const* mlp) {
  return SemW{uniform_ro(mlp[0]), uniform_ro(mlp[1]), uniform_ro(mlp[2]), uniform_ro(mlp[3]), uniform_ro(mlp[4]),
              uniform_ro(mlp[5])};
}

// h1 = relu(W1 f + b1) (registers), h2 = relu(W2 h1 + b2) (staged at row[0..32)); the ReLU masks.  row: the lane's own LDS
// row (>= 32 floats); h1 passes through it first.
__device__ __forceinline__ void sem_hidden(const SemW& w, const float (&f)[F], float* row, float (&h1)[H], unsigned& m1,
                                           unsigned& m2) {
  const int rows = opaque(H);
  m1 = 0u, m2 = 0u;
TERM_ROW_LOOP(4)
  for (int k = 0; k < rows; ++k) {
    float z = w.B1[k];
#pragma unroll
    for (int q = 0; q < F; ++q) z = fmaf(w.W1[k * F + q], f[q], z);
    m1 |= (z > 0.f ? 1u : 0u) << k;
    row[k] = fmaxf(z, 0.f);
  }
  wave_lds_fence();
#pragma unroll
  for (int k = 0; k < H; ++k) h1[k] = row[k];
  wave_lds_fence();
TERM_ROW_LOOP(2)
  for (int j = 0; j < rows; ++j) {
    float z = w.B2[j];
#pragma unroll
    for (int k = 0; k < H; ++k) z = fmaf(w.W2[j * H + k], h1[k], z);
    m2 |= (z > 0.f ? 1u : 0u) << j;
    row[j] = fmaxf(z, 0.f);
  }
  wave_lds_fence();
}

// z = Wc h2 + bc (h2 at row[0..32)) -> logp into row[0..C); returns the argmax of the rounded logp (first index on ties)
__device__ __forceinline__ int sem_head(const SemW& w, float* row, int C) {
  float h2[H];
#pragma unroll
  for (int k = 0; k < H; ++k) h2[k] = row[k];
  wave_lds_fence();
  const int nc = opaque(C);
  float mx = -__builtin_inff();
TERM_ROW_LOOP(2)
  for (int c = 0; c < nc; ++c) {
    float z = w.BC[c];
#pragma unroll
    for (int k = 0; k < H; ++k) z = fmaf(w.WC[c * H + k], h2[k], z);
    row[c] = z;
    mx = fmaxf(mx, z);
  }
  wave_lds_fence();
  float s = 0.f;
  for (int c = 0; c < nc; ++c) s += expf(row[c] - mx);
  const float lse = logf(s);
  int best = 0;
  float bv = 0.f;
  for (int c = 0; c < nc; ++c) {
    const float lp = (row[c] - mx) - lse;
    row[c] = lp;
    if (c == 0 || lp > bv) bv = lp, best = c;  // (strictly greater: the first of equal values wins, torch.argmax's rule)
  }
  return best;
}

// where element k of a partial vector lands in the six gradient tensors (null: padding behind the C classes of Wc / bc)
__device__ __forceinline__ float* sem_grad_slot(const SemGradPtrs& gp, int k, int C) {
  if (k < P_B1) return gp.g[0] + (k - P_W1);
  if (k < P_W2) return gp.g[1] + (k - P_B1);
  if (k < P_B2) return gp.g[2] + (k - P_W2);
  if (k < P_WC) return gp.g[3] + (k - P_B2);
  if (k < P_BC) return k - P_WC < C * H ? gp.g[4] + (k - P_WC) : nullptr;
  return k - P_BC < C ? gp.g[5] + (k - P_BC) : nullptr;
}

// The grid sum (grid_sum_two_level) of the workgroups' partial vectors, STRIDE floats each at ws + kCounterBytes, the run sums
// behind them: every summed element is stored to (ADD: added to) its place in the six tensors of gp.  With STRIDE = P_N + 4 the
// float at P_N is summed along and *loss_out = its sum * loss_scale (the three floats behind it are summed along and never used).
// A frozen head (!wgrad): only the loss's column is summed.  The partials are left as they are: every launch stores all it reads.
template <int STRIDE, bool ADD>
__device__ __forceinline__ void sem_grid_sum(unsigned char* ws, bool wgrad, const SemGradPtrs& gp, int C, float* loss_out,
                                             float loss_scale, unsigned* verdict) {
  static_assert((STRIDE == P_N || STRIDE == P_N + 4) && P_N % 4 == 0 && P_B1 % 4 == 0 && P_BC % 4 == 0, "float4 walk");
  float* part = reinterpret_cast<float*>(ws + kCounterBytes);
  const GridSumWs w = {reinterpret_cast<unsigned*>(ws), part, part + (size_t)kMaxBlocks * STRIDE, nullptr, nullptr};
  grid_sum_two_level<STRIDE, P_N / 4, false, 0>(
      w, wgrad, verdict,
      [&](int k, float4 s) {
        if (k == P_N) {
          loss_out[0] = s.x * loss_scale;
          return;
        }
        const float sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float* dst = sem_grad_slot(gp, k + e, C);
          if (dst) *dst = ADD ? *dst + sv[e] : sv[e];
        }
      },
      [](const double*) {});
}

inline int fill_mlp(SemArgsPtrs* p, const float* const* mlp, int32_t n_class, const char* what) {
  if (!mlp || n_class < 1 || n_class > CM) return set_error(SHINE_E_INVALID, what);
  for (int k = 0; k < 6; ++k) {
    if (!mlp[k]) return set_error(SHINE_E_INVALID, what);
    p->mlp[k] = mlp[k];
  }
  return SHINE_OK;
}

}  // namespace sem
}  // namespace shine
