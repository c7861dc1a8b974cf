// shine_draw_rider.hpp — cfg->draw_rider (include/shine_hip.h shine_draw_rider) as a device function: the whole next sorted draw
// and the next step's zero-fill, run by extra workgroups of a launch that has other work to do.  Two hosts:
//   * k_reduce_partials (shine_step_support.hip), 1024 threads = 4 sampler blocks per workgroup: the rider of a step whose record
//     carries no idx_next;
//   * k_step_v3 (shine_step_v3.hip), 512 / 256 threads = 2 / 1 sampler blocks per workgroup: trailing workgroups of the FUSED
//     launch (DrawRiderArgs::on_tail).  They need the registers and LDS of a step workgroup, so the dispatcher places them where a
//     step workgroup has retired: the draw runs in the launch's ragged end instead of behind it.
#pragma once
#include "shine_sampler_dev.hpp"
#include "shine_step_common.hpp"

namespace shine {

// One workgroup of Q x 256 threads = Q sampler blocks of 256 threads (quarter q = threadIdx.x >> 8).  The first ceil(nblocks / Q)
// rider workgroups run pass 1 of the draw after next, the others pass 2 of the next draw — k_sample_pass1 / k_sample_pass2's
// arithmetic and summation order (shine_sampler.hip), so the draws are bit-identical to the stand-alone sampler's; every rider
// thread also takes its share of the zero-fill.  `rb`: index among the rider workgroups.  `idx`: where pass 2 writes the draw.
// `clear_this`: also clear parts_this (only where this step's fused kernel is known to have read it: not on the fused launch).
// No workgroup waits for another: s_red / s_wave_pre / s_cnt are per workgroup, the barriers are workgroup barriers.
template <int Q>
__device__ __forceinline__ void draw_rider_block(const DrawRiderArgs& dr, int rb, int* idx, bool clear_this) {
  __shared__ double s_red[Q][4];
  __shared__ double s_wave_pre[Q][4];
  __shared__ int s_cnt[Q][4];
  const int qb = (dr.nblocks + Q - 1) / Q;
  const int q = threadIdx.x >> 8, t256 = threadIdx.x & 255, w = t256 >> 6, lane = threadIdx.x & 63;
  const unsigned long long sid = dr.state[dr.parity];  // stream id of the draw THIS step used
  for (long long z = (long long)rb * (Q * 256) + threadIdx.x; z < dr.zero_n16; z += (long long)2 * qb * (Q * 256))
    dr.zero_ptr[z] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (rb < qb) {  // ---- pass 1 of draw sid + 2
    const unsigned long long stream = sid + 2ull;
    const int vb = rb * Q + q;
    if (rb == 0 && threadIdx.x == 0) dr.state[1 - dr.parity] = sid + 1ull;
    if (clear_this && rb == 0 && dr.parts_this && threadIdx.x < SURF_PARTS) dr.parts_this[threadIdx.x] = 0;
    const long long k0 = (long long)vb * SB + t256 * 4;
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (vb < dr.nblocks && k0 + j < dr.n + 1) v += exp1v(dr.seed, stream, (unsigned long long)(k0 + j));
    v = wave_sum_d(v);
    if (lane == 0) s_red[q][w] = v;
    __syncthreads();
    if (t256 == 0 && vb < dr.nblocks) dr.bs_after[vb] = s_red[q][0] + s_red[q][1] + s_red[q][2] + s_red[q][3];
    return;
  }
  // ---- pass 2 of draw sid + 1
  const unsigned long long stream = sid + 1ull;
  const int vb = (rb - qb) * Q + q;
  const bool on = vb < dr.nblocks;  // (padding quarters of the last block walk through the barriers only)
  double before = 0.0, total = 0.0;
  for (int b = t256; b < dr.nblocks; b += 256) {
    const double v = dr.bs_next[b];
    total += v;
    if (b < vb) before += v;
  }
  before = wave_sum_d(before);
  if (lane == 0) s_red[q][w] = before;
  __syncthreads();
  before = s_red[q][0] + s_red[q][1] + s_red[q][2] + s_red[q][3];
  __syncthreads();
  total = wave_sum_d(total);
  if (lane == 0) s_red[q][w] = total;
  __syncthreads();
  total = s_red[q][0] + s_red[q][1] + s_red[q][2] + s_red[q][3];
  __syncthreads();
  const long long k0 = (long long)vb * SB + t256 * 4;
  double e[4], run = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    e[j] = (on && k0 + j <= dr.n) ? exp1v(dr.seed, stream, (unsigned long long)(k0 + j)) : 0.0;
    run += e[j];
  }
  double inc = run;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  if (lane == 63) s_wave_pre[q][w] = inc;
  __syncthreads();
  double wpre = 0.0;
  for (int ww = 0; ww < w; ++ww) wpre += s_wave_pre[q][ww];
  double sacc = before + wpre + (inc - run);
  int surf = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    sacc += e[j];
    if (on && k0 + j < dr.n) {
      long long v = (long long)((sacc / total) * (double)dr.pool);
      v = v < 0 ? 0 : (v >= dr.pool ? dr.pool - 1 : v);
      idx[k0 + j] = (int)v;
      if (dr.parts_next) surf += (int)((dr.surf_bits[v >> 5] >> (v & 31)) & 1u);
    }
  }
  if (dr.parts_next) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) surf += __shfl_xor(surf, o, 64);
    if (lane == 0) s_cnt[q][w] = surf;
    __syncthreads();
    if (t256 == 0 && on)
      __hip_atomic_fetch_add(dr.parts_next + (vb & (SURF_PARTS - 1)), (long long)(s_cnt[q][0] + s_cnt[q][1] + s_cnt[q][2] + s_cnt[q][3]),
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// workgroups a rider of Q sampler blocks per workgroup adds to its launch: pass 1 and pass 2, ceil(nblocks / Q) each
inline int draw_rider_workgroups(int nblocks, int q) { return 2 * ((nblocks + q - 1) / q); }

}  // namespace shine
