// shine_sem_head.hpp — the semantic head's device code shared by shine_semantic.hip (forward, backward, mesh labels) and
// shine_sem_step.hip (the training loop's NLL launch): the weight pointers, the two hidden layers, the class layer with its
// log-softmax, and the layout of the per-workgroup weight-grad partials that the ticket reduction sums.
#pragma once
#include "shine_internal.hpp"

namespace shine {
namespace sem {

constexpr int CM = SHINE_SEM_MAX_CLASSES;  // 32
constexpr int SR = 33;                     // forward staging row stride (odd: the lanes' rows hit different banks)
constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256;            // backward workgroups at most
constexpr int kGroup = 16;                 // workgroups per first-level run
constexpr int kGroups = kMaxBlocks / kGroup;
// partial layout (floats): W1 [32][8] | b1 [32] | W2 [32][32] | b2 [32] | Wc [32][32] | bc [32] (Wc / bc padded to 32 classes)
constexpr int P_W1 = 0, P_B1 = P_W1 + H * F, P_W2 = P_B1 + H, P_B2 = P_W2 + H * H, P_WC = P_B2 + H, P_BC = P_WC + CM * H;
constexpr int P_N = P_BC + CM;
constexpr size_t kCounterBytes = 256;  // [0] run-level ticket, [1..kGroups] first-level tickets
static_assert(kCounterBytes + (size_t)(kMaxBlocks + kGroups) * P_N * sizeof(float) <= SHINE_SEM_WORKSPACE_BYTES, "workspace");
static_assert((kGroups + 1) * sizeof(unsigned) <= kCounterBytes, "counters");

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

#define SEM_LOOP_STR(x) #x
#define SEM_ROW_LOOP(n) _Pragma(SEM_LOOP_STR(clang loop vectorize(disable) interleave(disable) unroll_count(n)))

// h1 = relu(W1 f + b1) (registers), h2 = relu(W2 h1 + b2) (staged at row[0..32)); the ReLU masks.  row: the lane's own LDS
// row (>= 32 floats); h1 passes through it first.
__device__ __forceinline__ void sem_hidden(const SemW& w, const float (&f)[F], float* row, float (&h1)[H], unsigned& m1,
                                           unsigned& m2) {
  const int rows = opaque(H);
  m1 = 0u, m2 = 0u;
SEM_ROW_LOOP(4)
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
SEM_ROW_LOOP(2)
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
SEM_ROW_LOOP(2)
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
