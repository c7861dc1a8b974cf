// shine_term_host.hpp — the host side every term step shares (shine_sem_step.hip, shine_normal_step.hip,
// shine_consistency_step.hip): the refusals that keep a bad pointer out of a launch, the level descriptors, the
// answer for an empty batch, and the (L, interpolation) dispatch the query entry points use too.  Host only: no device code.
//
// An entry point runs term_prologue, term_decoder (or the head's own fill_mlp + term_wgrads), its term's refusals and
// term_levels, then either term_empty or dispatch_levels_poly around ITS launch.  Every refusal comes before anything is enqueued.
#pragma once
#include <cstdio>
#include <type_traits>

#include "shine_internal.hpp"

namespace shine {

// "<entry>: <what>" as SHINE_E_INVALID (set_error copies the text)
inline int term_refuse(const char* entry, const char* what) {
  char msg[192];
  snprintf(msg, sizeof(msg), "%s: %s", entry, what);
  return set_error(SHINE_E_INVALID, msg);
}

// The arguments every term step has.
inline int term_prologue(const char* entry, const shine_tables* t, const shine_step_config* cfg, int32_t coord_stride, int64_t n,
                         const float* const* feats, const int64_t* rows, const float* loss_out, const void* workspace) {
  if (!t) return term_refuse(entry, "null table handle");
  if (!cfg) return term_refuse(entry, "null config");
  if (coord_stride != 3 && coord_stride != 8)
    return term_refuse(entry, "coord_stride is 3 ([n,3] array) or 8 (32-byte pool records)");
  if (n < 0) return term_refuse(entry, "n < 0");
  if (!feats || !rows || !loss_out) return term_refuse(entry, "null argument");
  if (!workspace || ((size_t)workspace & 255)) return term_refuse(entry, "workspace");
  return SHINE_OK;
}

// The levels into *ls, after every refusal that needs no table (a handle without tables is a STATE error, reported last): the
// kernels are built for 1..4 levels and index a level's rows with 32 bits (id * 8 + feature).
inline int term_levels(const char* entry, const shine_tables* t, const shine_step_config* cfg, const float* const* feats,
                       const int64_t* rows, float* const* grad_feats, LevelSet* ls) {
  if (cfg->n_levels > 4) return term_refuse(entry, "more than 4 featured levels");
  const int rc = make_level_set(t, cfg, feats, rows, grad_feats, ls);
  if (rc != SHINE_OK) return rc;
  for (int s = 0; s < cfg->n_levels; ++s) {
    if (!feats[s]) return term_refuse(entry, "null feature level");
    if (rows[s] >= (1ll << 29)) return term_refuse(entry, "level exceeds 2^29 rows");
  }
  return SHINE_OK;
}

// grad_mlp: NULL (a frozen decoder) or six tensors
inline int term_wgrads(const char* entry, float* const* grad_mlp) {
  for (int k = 0; grad_mlp && k < 6; ++k)
    if (!grad_mlp[k]) return term_refuse(entry, "null weight-grad tensor");
  return SHINE_OK;
}

// The geometry decoder's six tensors and its weight grads into a term's Args (mlp[6], gW1, gW2, gw3, want_wgrad).
template <class Args>
int term_decoder(const char* entry, const float* const* mlp, float* const* grad_mlp, Args* a) {
  if (!mlp) return term_refuse(entry, "null argument");
  for (int k = 0; k < 6; ++k) {
    if (!mlp[k]) return term_refuse(entry, "null decoder parameter");
    a->mlp[k] = mlp[k];
  }
  const int rc = term_wgrads(entry, grad_mlp);
  if (rc != SHINE_OK) return rc;
  if (grad_mlp) a->gW1 = grad_mlp[0], a->gW2 = grad_mlp[2], a->gw3 = grad_mlp[4];  // (the three biases receive nothing)
  a->want_wgrad = grad_mlp ? 1 : 0;
  return SHINE_OK;
}

// An empty batch: the loss is 0 and nothing else is written.
inline int term_empty(float* loss_out, hipStream_t st) {
  SHINE_HIP_CHECK(hipMemsetAsync(loss_out, 0, sizeof(float), st));
  return SHINE_OK;
}

// f(std::integral_constant<int, L>, std::bool_constant<POLY>) for L in 1..4; false (f not called): L is out of that range.
template <class F>
bool dispatch_levels_poly(int L, bool poly, F&& f) {
  auto with = [&](auto l) { poly ? f(l, std::true_type{}) : f(l, std::false_type{}); };
  switch (L) {
    case 1: with(std::integral_constant<int, 1>{}); return true;
    case 2: with(std::integral_constant<int, 2>{}); return true;
    case 3: with(std::integral_constant<int, 3>{}); return true;
    case 4: with(std::integral_constant<int, 4>{}); return true;
    default: return false;
  }
}

}  // namespace shine
