// shine_mlp_body.hpp — k_mlp_bwd: the backward and backward-backward of the Tier A decoder op, shared by Decoder.sdf
// (shine_mlp.hip, TIME = false: W1 [32][8]) and Decoder.time_conditionded_sdf (shine_time_mlp.hip, TIME = true: W1 [32][9] read
// in place, one scalar `ts` per point).  The time input is a per-point shift of the first bias, z1 = W1f f + (b1 + w_t ts): it moves the
// ReLU masks and adds ONE weight-grad column, dW1[:,8] += sum_i ts_i d1_i, to the first backward; the backward-backward sees it
// through the masks alone.  Every TIME branch is `if constexpr`: the TIME = false instantiations keep the register, LDS and
// scratch figures the kernels had without the time input (profiles/time_decoder_resources.txt).
#pragma once
#include <type_traits>

#include "shine_internal.hpp"

namespace shine {

struct MlpArgs {
  const float* feat;    // [n][8]
  const float* g;       // [n] d loss / d pred                      (modes 1, 2)
  const float* r;       // [n][8] d loss / d(grad_feat)             (mode 2)
  const float* mlp[6];
  float* pred;          // [n]                                      (mode 0)
  float* grad_feat;     // [n][8] or null                           (mode 1)
  float* grad_g;        // [n] or null                              (mode 2)
  float* grad_mlp[6];   // accumulated into, or all null
  long long n;
  int want_wgrad;
};

struct TimeMlpArgs : MlpArgs {
  const float* ts;      // [n] the time input of every point; mlp[0] / grad_mlp[0] are [32][9]
};

// a rolled loop over weight rows: opaque trip count (device.hpp), and keep the loop vectoriser away from it
#define ROW_LOOP_STR(x) #x
#define ROW_LOOP(n) _Pragma(ROW_LOOP_STR(clang loop vectorize(disable) interleave(disable) unroll_count(n)))

// ---- backward (MODE 1) and backward-backward (MODE 2): one wave = one 64-point tile at a time, lane = point.
// The layers are ROLLED loops over the weight rows (an unrolled 32x32 layer let the compiler keep a thousand loaded
// weights live and spill them); register arrays are only ever indexed statically (h1 / d1 / v1 / a1 inside the row
// loops), per-row results that a rolled loop produces go through the lane's own LDS staging row — the same rows the
// weight-grad contractions over the tile's 64 points read afterwards.  Nothing is shared between waves: DS operations of
// one wave execute in order, so the hand-offs need no workgroup barrier.
// IN: the row stride of W1 (TIME: its rows are not 16-byte aligned — scalar loads only, no float4).
template <int MODE, bool TIME = false>
__global__ __launch_bounds__(256) void k_mlp_bwd(std::conditional_t<TIME, TimeMlpArgs, MlpArgs> a) {
  __shared__ float s_stage[4 * 64 * ST];
  constexpr int IN = TIME ? F + 1 : F;
  cfloat *const W1 = uniform_ro(a.mlp[0]), *const B1 = uniform_ro(a.mlp[1]), *const W2 = uniform_ro(a.mlp[2]),
               *const B2 = uniform_ro(a.mlp[3]), *const W3 = uniform_ro(a.mlp[4]);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* st = s_stage + wv * 64 * ST;
  float* row = st + lane * ST;  // [0,32) left operands, [32,64) right operands, [64,75) spare

  float accW2[16], accW1[4];
  float accb2 = 0.f, accb1 = 0.f, accw3 = 0.f, accb3 = 0.f;
  float accWt = 0.f;  // (TIME, mode 1) dW1[jj][8]
#pragma unroll
  for (int q = 0; q < 16; ++q) accW2[q] = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) accW1[q] = 0.f;
  const int jj = lane & 31, hi = lane >> 5;
  const bool wgrad = a.want_wgrad;

  const long long tiles = (a.n + 63) >> 6;
  const int rows = opaque(H);
  for (long long t = (long long)blockIdx.x * 4 + wv; t < tiles; t += (long long)gridDim.x * 4) {
    const long long i = t * 64 + lane;
    const bool valid = i < a.n;
    float f[F];
#pragma unroll
    for (int q = 0; q < F; ++q) f[q] = 0.f;
    float g = 0.f;  // padding lanes contribute zeros to the contractions
    float ts = 0.f;
    if (valid) {
      const float4* fr = reinterpret_cast<const float4*>(a.feat + i * F);
      const float4 r0 = fr[0], r1 = fr[1];
      f[0] = r0.x, f[1] = r0.y, f[2] = r0.z, f[3] = r0.w, f[4] = r1.x, f[5] = r1.y, f[6] = r1.z, f[7] = r1.w;
      g = a.g[i];
      if constexpr (TIME) ts = a.ts[i];
    }
    // ---- forward, recomputed (8 floats in, nothing saved between passes): ReLU masks m1 / m2, h1 in registers
    unsigned int m1 = 0u, m2 = 0u;
ROW_LOOP(4)
    for (int k = 0; k < rows; ++k) {
      float z = B1[k];
      if constexpr (TIME) z = fmaf(W1[k * IN + F], ts, z);
#pragma unroll
      for (int q = 0; q < F; ++q) z = fmaf(W1[k * IN + q], f[q], z);
      m1 |= (z > 0.f ? 1u : 0u) << k;
      row[32 + k] = fmaxf(z, 0.f);
    }
    wave_lds_fence();
    float h1[H];
#pragma unroll
    for (int k = 0; k < H; ++k) h1[k] = row[32 + k];
ROW_LOOP(2)
    for (int j = 0; j < rows; ++j) {
      float z = B2[j];
#pragma unroll
      for (int k = 0; k < H; ++k) z = fmaf(W2[j * H + k], h1[k], z);
      m2 |= (z > 0.f ? 1u : 0u) << j;
      if (MODE == 1 && wgrad) row[j] = g * fmaxf(z, 0.f);
    }

    if (MODE == 1) {
      if (wgrad) {  // dw3 += g h2
        wave_lds_fence();
        _Pragma("clang loop vectorize(disable) interleave(disable) unroll_count(8)")
        for (int pp = 0; pp < 64; ++pp) accw3 += st[pp * ST + jj];
        wave_lds_fence();
      }
      // ---- d2 = g (m2 .* w3);  d1 = m1 .* W2^T d2;  df = W1^T d1
      float d1[H];
#pragma unroll
      for (int k = 0; k < H; ++k) d1[k] = 0.f;
ROW_LOOP(2)
      for (int j = 0; j < rows; ++j) {
        const float d2 = ((m2 >> j) & 1u) ? g * W3[j] : 0.f;
        if (wgrad) row[j] = d2;
#pragma unroll
        for (int k = 0; k < H; ++k) d1[k] = fmaf(W2[j * H + k], d2, d1[k]);
      }
      if (wgrad) {  // dW2 += d2 (x) h1 ; db2 += d2     (h1 is still staged at [32,64))
        wave_lds_fence();
        contract64r<16>(st, jj, 32 + hi * 16, accW2, accb2, true);
        wave_lds_fence();
      }
#pragma unroll
      for (int k = 0; k < H; ++k) row[k] = ((m1 >> k) & 1u) ? d1[k] : 0.f;
#pragma unroll
      for (int q = 0; q < F; ++q) row[32 + q] = f[q];
      row[40] = g;
      if constexpr (TIME) row[41] = ts;
      wave_lds_fence();
      float df[F];
#pragma unroll
      for (int q = 0; q < F; ++q) df[q] = 0.f;
ROW_LOOP(8)
      for (int k = 0; k < rows; ++k) {
        const float dk = row[k];
#pragma unroll
        for (int q = 0; q < F; ++q) df[q] = fmaf(W1[k * IN + q], dk, df[q]);
      }
      if (valid && a.grad_feat) {
        float4* o = reinterpret_cast<float4*>(a.grad_feat + i * F);
        o[0] = make_float4(df[0], df[1], df[2], df[3]);
        o[1] = make_float4(df[4], df[5], df[6], df[7]);
      }
      if (wgrad) {  // dW1[:, :8] += d1 (x) f ; db1 += d1 ; db3 += g ; (TIME) dW1[:, 8] += d1 ts
        contract64r<4>(st, jj, 32 + hi * 4, accW1, accb1, true);
        _Pragma("clang loop vectorize(disable) interleave(disable) unroll_count(8)")
        for (int pp = 0; pp < 64; ++pp) {
          accb3 += st[pp * ST + 40];
          if constexpr (TIME) accWt = fmaf(st[pp * ST + jj], st[pp * ST + 41], accWt);
        }
        wave_lds_fence();
      }
    } else {
      // ---- v2 = m2 .* w3;  v1 = m1 .* W2^T v2;  J = W1^T v1;  a1 = m1 .* W1 r;  a2 = m2 .* W2 a1
      //      (TIME: r has no time component — ts gets no gradient — so W1 r reads the first eight columns only)
      float rr[F];
#pragma unroll
      for (int q = 0; q < F; ++q) rr[q] = 0.f;
      if (valid) {
        const float4* rp = reinterpret_cast<const float4*>(a.r + i * F);
        const float4 r0 = rp[0], r1 = rp[1];
        rr[0] = r0.x, rr[1] = r0.y, rr[2] = r0.z, rr[3] = r0.w, rr[4] = r1.x, rr[5] = r1.y, rr[6] = r1.z, rr[7] = r1.w;
      }
      float v1[H];
#pragma unroll
      for (int k = 0; k < H; ++k) v1[k] = 0.f;
ROW_LOOP(2)
      for (int j = 0; j < rows; ++j) {
        const float v2 = ((m2 >> j) & 1u) ? W3[j] : 0.f;
        if (wgrad) row[j] = g * v2;
#pragma unroll
        for (int k = 0; k < H; ++k) v1[k] = fmaf(W2[j * H + k], v2, v1[k]);
      }
      // t = W1 r, one row of W1 at a time, through the staging row (h1 is no longer needed there)
ROW_LOOP(4)
      for (int k = 0; k < rows; ++k) {
        float tk = 0.f;
#pragma unroll
        for (int q = 0; q < F; ++q) tk = fmaf(W1[k * IN + q], rr[q], tk);
        row[32 + k] = tk;
      }
      wave_lds_fence();
      float gj = 0.f;  // r . J = sum_k v1[k] (W1 r)[k]
      float a1[H];
#pragma unroll
      for (int k = 0; k < H; ++k) {
        const bool on = (m1 >> k) & 1u;
        const float tk = row[32 + k];
        v1[k] = on ? v1[k] : 0.f;
        gj = fmaf(v1[k], tk, gj);
        a1[k] = on ? tk : 0.f;
      }
      if (valid && a.grad_g) a.grad_g[i] = gj;
      if (wgrad) {
        // dW2 += (g v2) (x) a1
#pragma unroll
        for (int k = 0; k < H; ++k) row[32 + k] = a1[k];
        wave_lds_fence();
        float dummy = 0.f;
        contract64r<16>(st, jj, 32 + hi * 16, accW2, dummy, false);
        wave_lds_fence();
        // dW1[:, :8] += (g v1) (x) r ; dw3 += g a2
#pragma unroll
        for (int k = 0; k < H; ++k) row[k] = g * v1[k];
#pragma unroll
        for (int q = 0; q < F; ++q) row[32 + q] = rr[q];
ROW_LOOP(2)
        for (int j = 0; j < rows; ++j) {
          float tj = 0.f;
#pragma unroll
          for (int k = 0; k < H; ++k) tj = fmaf(W2[j * H + k], a1[k], tj);
          row[40 + j] = ((m2 >> j) & 1u) ? g * tj : 0.f;
        }
        wave_lds_fence();
        contract64r<4>(st, jj, 32 + hi * 4, accW1, dummy, false);
        _Pragma("clang loop vectorize(disable) interleave(disable) unroll_count(8)")
        for (int pp = 0; pp < 64; ++pp) accw3 += st[pp * ST + 40 + jj];
        wave_lds_fence();
      }
    }
  }

  if (wgrad) {
    // One flush per WORKGROUP: the 1377 (TIME: 1409) targets are the same for every wave of the launch, and same-address fp32
    // atomics retire at ~3 per ns in total (measured: 1024 waves x 1377 atomics took 0.5 ms, the arithmetic ~20 us) — so the
    // four waves are summed through LDS first and the grid is kept small (mlp_bwd_grid).
    __syncthreads();  // every wave is done with its staging rows
    constexpr int NV = (TIME && MODE == 1) ? 25 : 24;
    float vals[NV];
#pragma unroll
    for (int q = 0; q < 16; ++q) vals[q] = accW2[q];
#pragma unroll
    for (int q = 0; q < 4; ++q) vals[16 + q] = accW1[q];
    vals[20] = accw3, vals[21] = accb1, vals[22] = accb2, vals[23] = accb3;
    if constexpr (NV == 25) vals[24] = accWt;
#pragma unroll
    for (int v = 0; v < NV; ++v) s_stage[(wv * NV + v) * 64 + lane] = vals[v];
    __syncthreads();
    if (wv == 0) {
#pragma unroll
      for (int v = 0; v < NV; ++v)
        vals[v] = (s_stage[v * 64 + lane] + s_stage[(NV + v) * 64 + lane]) +
                  (s_stage[(2 * NV + v) * 64 + lane] + s_stage[(3 * NV + v) * 64 + lane]);
#pragma unroll
      for (int q = 0; q < 16; ++q) atomic_add_f32(a.grad_mlp[2] + jj * H + hi * 16 + q, vals[q]);
#pragma unroll
      for (int q = 0; q < 4; ++q) atomic_add_f32(a.grad_mlp[0] + jj * IN + hi * 4 + q, vals[16 + q]);
      if (hi == 0) {
        atomic_add_f32(a.grad_mlp[4] + jj, vals[20]);
        if (MODE == 1) {  // the eikonal pass sends nothing to the biases — nor, TIME, to the time column of W1
          atomic_add_f32(a.grad_mlp[1] + jj, vals[21]);
          atomic_add_f32(a.grad_mlp[3] + jj, vals[22]);
          if constexpr (NV == 25) atomic_add_f32(a.grad_mlp[0] + jj * IN + F, vals[24]);
          if (lane == 0) atomic_add_f32(a.grad_mlp[5], vals[23]);
        }
      }
    }
  }
}

// host side: the argument checks and the grids every entry point of the two files shares
static int fill_args(MlpArgs* a, const char* what, const float* feat, int64_t n, const float* const* mlp,
                     float* const* grad_mlp) {
  if (n < 0 || !mlp || (n > 0 && !feat)) return set_error(SHINE_E_INVALID, what);
  a->feat = feat;
  a->n = n;
  a->want_wgrad = grad_mlp ? 1 : 0;
  for (int k = 0; k < 6; ++k) {
    if (!mlp[k]) return set_error(SHINE_E_INVALID, what);
    a->mlp[k] = mlp[k];
    if (grad_mlp) {
      if (!grad_mlp[k]) return set_error(SHINE_E_INVALID, what);
      a->grad_mlp[k] = grad_mlp[k];
    }
  }
  return SHINE_OK;
}

static unsigned mlp_grid(int64_t n) {
  const long long b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

// backward launches that accumulate weight grads: every workgroup ends with 1377 atomics on the same addresses
// (~0.5 us per workgroup, serialised), a 64-point tile costs a wave ~10 us -> at most 96 workgroups
static unsigned mlp_bwd_grid(int64_t n, bool wgrad) {
  const unsigned g = mlp_grid(n);
  return (wgrad && g > 96u) ? 96u : g;
}

}  // namespace shine
