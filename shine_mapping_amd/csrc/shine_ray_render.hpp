// shine_ray_render.hpp — the per-ray arithmetic of batch_ray_rendering_loss (utils/loss.py:82-118), one sample at a time, shared
// by the Tier A loss (k_ray_render_loss, shine_loss_modes.hip: an unrolled register network) and the ray step (k_ray_step,
// shine_ray_step.hip: a runtime-S walk through LDS), so the two cannot drift apart.
//
// In depth order, with alphas a (the probabilities of dr, the clamped quotient of neighbours of dr_neus):
//   o = (1 - a) + 1e-10,  c = cumprod(o) (accumulated in fp64 as torch's CPU kernel does),  w = (c / o) a,  d = sum w x
// and the backward for an upstream gradient gd of d walks the samples from the far end (the reversed cumsum of cumprod's backward).
// The composite rounds every product and sum on its own; so does every function here (no a * b + c contracted into one rounding):
// saturated rays (a probability of exactly 0 or 1) make the autograd form of the gradient a difference of ~1e10-sized terms whose
// result depends on each of those roundings.
#pragma once
#include "shine_internal.hpp"

namespace shine {

// sort key: padding columns (>= S) last, then x with NaN after every number (torch.sort's order), then the column — ties are
// broken by the column, so any network gives the stable order, and the S real columns always fill positions 0..S-1
__device__ __forceinline__ bool ray_key_gt(float xa, int ia, float xb, int ib, int S) {
  const bool pa = ia >= S, pb = ib >= S;
  if (pa != pb) return pa;
  const bool na = xa != xa, nb = xb != xb;
  if (na != nb) return na;
  if (!na && xa != xb) return xa > xb;
  return ia > ib;
}

// dr_neus: the alpha of a sample from its own probability y0 and the next sample's y1 (the clamp's ends are closed)
__device__ __forceinline__ float ray_neus_alpha(float y0, float y1) {
#pragma clang fp contract(off)
  const float q = (y1 - y0) / ((1.0f - y0) + 1e-10f);
  return fminf(fmaxf(q, 0.f), 1.f);
}

// forward of one sample, nearest first: o and c of alpha a, the running fp64 product cp, d += w x
__device__ __forceinline__ void ray_forward(float a, float x, double& cp, float& o, float& c, float& d) {
#pragma clang fp contract(off)
  o = (1.0f - a) + 1e-10f;
  cp *= (double)o;
  c = (float)cp;
  d += ((c / o) * a) * x;
}

// d (mean |d - d_meas|) / d d for one ray (sgn(0) = 0)
__device__ __forceinline__ float ray_err_grad(float err, float inv_r) {
#pragma clang fp contract(off)
  return inv_r * (err > 0.f ? 1.f : (err < 0.f ? -1.f : 0.f));
}

// backward of one sample, farthest first: -> d loss / d a.  rc: the running fp64 reversed cumsum; `single`: the ray has ONE alpha
// (torch returns the gradient itself for a length-1 cumprod)
__device__ __forceinline__ float ray_backward(float gd, float x, float a, float o, float c, double& rc, bool single) {
#pragma clang fp contract(off)
  const float gw = gd * x;
  const float qq = c / o;
  const float gqq = gw * a;
  const float ga = gw * qq;
  const float gc = gqq / o;
  const float go_div = -gqq * (qq / o);
  rc += (double)(gc * c);
  const float go_cum = single ? gc : (float)rc / o;
  return ga + -(go_cum + go_div);
}

// dr_neus: d loss / d a through the clamp and the quotient -> gnum (ADDED to the next sample's gradient) and the sample's own
__device__ __forceinline__ void ray_neus_backward(float y0, float y1, float ga, float& gnum, float& gown) {
#pragma clang fp contract(off)
  const float num = y1 - y0;
  const float den = (1.0f - y0) + 1e-10f;
  const float q = num / den;
  const float gq = (q >= 0.f && q <= 1.f) ? ga : 0.f;
  gnum = gq / den;
  const float gden = -gq * (q / den);
  gown = -gnum + -gden;
}

}  // namespace shine
