// shine_frame.hip — the frame front-end of LiDARDataset.process_frame (dataset/lidar_dataset.py:115-290, utils/data_sampler.py:18-139)
// on the device: what turns one scan and one pose into training samples.
//   shine_frame_filter        preprocess_kitti (z > min_z, |p| >= min_range) + the inclusive crop box, fp64, compacted in input order
//   shine_sem_frame_filter    preprocess_sem_kitti (|p| >= range_min, label < 100, label != 1) + the learning map + the inclusive crop
//                             box, fp64, points and classes compacted in input order, ONE launch
//   shine_depth_unproject     a depth image (uint16 / float32) -> the frame's points: back-projection through the pinhole intrinsics
//                             (dataset/rgbd_to_kitti_format.py:78-81), the camera-to-sensor matrix and shine_frame_filter's test,
//                             compacted in pixel order, ONE launch
//   shine_ray_sample          dataSampler.sample: surface / clearance / free-space samples of every ray, ONE launch, ray-major
//   shine_pool_window_filter  the sliding window of the batch-mode pool (|coord - origin| < radius), stable, <= 6 parallel arrays
// All five are streaming kernels: the sampler writes 4-byte words lane-contiguously (the [*,3] rows go through LDS so that its
// stores are dword-linear too) and has no atomics; the four compactions order their tiles through one chained prefix
// (tile_exclusive_prefix) instead of a scan launch, so the input is read once.
#include "shine_internal.hpp"

namespace shine {
namespace {

constexpr int T = 256;  // threads per workgroup (4 waves)

// ---- stable compaction: the exclusive prefix of a tile's kept count over all tiles in front of it, inside the launch ----------
// Tiles are taken in TICKET order (one atomic counter), so every tile a workgroup waits for belongs to a workgroup that is already
// running: no assumption about dispatch order or co-residency.  A tile publishes ONE 64-bit word {status, value} — first its own
// count (AGGREGATE), after the look-back its inclusive prefix (PREFIX) — so value and flag cannot be seen apart.  Wave 0 looks
// back 64 tiles at a time and stops at the nearest PREFIX.  `state` (one word per tile) and `counter` are cleared by the host
// wrapper in front of every launch.
constexpr unsigned long long ST_AGG = 1ull << 62, ST_PREFIX = 2ull << 62, ST_VALUE = (1ull << 62) - 1ull;

struct TileShared {
  int cnt[32];
  int off[32];
  long long excl;
  int ticket;
};

__device__ __forceinline__ int take_ticket(TileShared& sm, unsigned int* counter) {
  if (threadIdx.x == 0) sm.ticket = (int)atomicAdd(counter, 1u);
  __syncthreads();
  return sm.ticket;
}

// all T threads call; returns the number of kept elements in tiles [0, tile)
__device__ __forceinline__ long long tile_exclusive_prefix(TileShared& sm, unsigned long long* state, int tile, long long count) {
  if (threadIdx.x == 0)
    __hip_atomic_store(state + tile, (tile == 0 ? ST_PREFIX : ST_AGG) | (unsigned long long)count, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    long long excl = 0;
    for (int j = tile - 1; j >= 0; j -= 64) {
      const int idx = j - lane;
      unsigned long long w = ST_PREFIX;  // (in front of tile 0: an empty prefix)
      if (idx >= 0) {
        w = __hip_atomic_load(state + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while ((w >> 62) == 0ull) {
          __builtin_amdgcn_s_sleep(1);
          w = __hip_atomic_load(state + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      const unsigned long long has_prefix = __ballot((w >> 62) == 2ull);
      const int first = has_prefix ? __ffsll((long long)has_prefix) - 1 : 63;  // nearest predecessor that knows its prefix
      long long v = lane <= first ? (long long)(w & ST_VALUE) : 0ll;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      excl += v;
      if (has_prefix) break;
    }
    if (lane == 0) {
      if (tile > 0)
        __hip_atomic_store(state + tile, ST_PREFIX | (unsigned long long)(excl + count), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      sm.excl = excl;
    }
  }
  __syncthreads();
  return sm.excl;
}

// Element k * T + thread of a tile of ITEMS * T elements (thread-strided: coalesced loads).  rank[k] = kept elements of the tile in
// front of that element (input order); returns the tile's kept count.
template <int ITEMS>
__device__ __forceinline__ int tile_ranks(TileShared& sm, const bool (&keep)[ITEMS], int (&rank)[ITEMS]) {
  static_assert(ITEMS * (T / 64) <= 32, "tile too large for TileShared");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned long long bal[ITEMS];
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    bal[k] = __ballot(keep[k]);
    if (lane == 0) sm.cnt[k * (T / 64) + wv] = __popcll(bal[k]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int e = 0; e < ITEMS * (T / 64); ++e) {
      sm.off[e] = run;
      run += sm.cnt[e];
    }
    sm.cnt[0] = run;
  }
  __syncthreads();
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) rank[k] = sm.off[k * (T / 64) + wv] + __popcll(bal[k] & below);
  return sm.cnt[0];
}

// ---- shine_frame_filter ------------------------------------------------------------------------------------------------------
constexpr int FI = 8;  // points per thread: a 64 x 450 scan is 15 tiles

struct FilterBox {
  double min_z, max_z, min_range, radius;
};

template <typename P>
__global__ __launch_bounds__(T) void k_frame_filter(const P* __restrict__ pts, int stride, long long n, FilterBox b,
                                                    double* __restrict__ out, unsigned long long* state, unsigned int* counter,
                                                    long long* total, int n_tiles) {
#pragma clang fp contract(off)  // (numpy's x*x + y*y + z*z has no fused multiply-add: the kept set is compared exactly)
  __shared__ TileShared sm;
  const int tile = take_ticket(sm, counter);
  const long long base = (long long)tile * (FI * T);
  double x[FI], y[FI], z[FI];
  bool keep[FI];
  int rank[FI];
#pragma unroll
  for (int k = 0; k < FI; ++k) {
    const long long i = base + k * T + threadIdx.x;
    keep[k] = false;
    if (i < n) {
      x[k] = (double)pts[i * stride];
      y[k] = (double)pts[i * stride + 1];
      z[k] = (double)pts[i * stride + 2];
      const double r = __dsqrt_rn(x[k] * x[k] + y[k] * y[k] + z[k] * z[k]);
      keep[k] = z[k] > b.min_z && r >= b.min_range && x[k] >= -b.radius && x[k] <= b.radius && y[k] >= -b.radius &&
                y[k] <= b.radius && z[k] >= b.min_z && z[k] <= b.max_z;
    }
  }
  const int count = tile_ranks<FI>(sm, keep, rank);
  const long long excl = tile_exclusive_prefix(sm, state, tile, count);
#pragma unroll
  for (int k = 0; k < FI; ++k)
    if (keep[k]) {
      double* o = out + (excl + rank[k]) * 3;
      o[0] = x[k];
      o[1] = y[k];
      o[2] = z[k];
    }
  if (tile == n_tiles - 1 && threadIdx.x == 0) *total = excl + count;
}

// ---- shine_sem_frame_filter ----------------------------------------------------------------------------------------------------
// k_frame_filter's sibling for a labelled scan (dataset/lidar_dataset.py:341-362, then the crop of :138-142): the label test runs on
// the raw 16-bit id, the kept points carry lut[id].  `unknown` counts the points that pass the label test with an id the map does
// not hold (the reference raises KeyError for those before it crops): one atomic per wave that saw any.
struct SemFilter {
  double range_min, min_z, max_z, radius;
  int filter_moving, filter_outlier;
};

template <typename P>
__global__ __launch_bounds__(T) void k_sem_frame_filter(const P* __restrict__ pts, int stride,
                                                        const unsigned int* __restrict__ labels, const int* __restrict__ lut,
                                                        long long n, SemFilter f, double* __restrict__ out,
                                                        int* __restrict__ class_out, unsigned long long* state,
                                                        unsigned int* counter, long long* total, unsigned long long* unknown,
                                                        int n_tiles) {
#pragma clang fp contract(off)  // (as k_frame_filter: the kept set is compared exactly with numpy's)
  __shared__ TileShared sm;
  const int tile = take_ticket(sm, counter);
  const long long base = (long long)tile * (FI * T);
  double x[FI], y[FI], z[FI];
  int cls[FI];
  bool keep[FI];
  int rank[FI];
  int n_unknown = 0;
#pragma unroll
  for (int k = 0; k < FI; ++k) {
    const long long i = base + k * T + threadIdx.x;
    keep[k] = false;
    cls[k] = 0;
    if (i < n) {
      x[k] = (double)pts[i * stride];
      y[k] = (double)pts[i * stride + 1];
      z[k] = (double)pts[i * stride + 2];
      const unsigned int s = labels[i] & 0xFFFFu;
      const double r = __dsqrt_rn(x[k] * x[k] + y[k] * y[k] + z[k] * z[k]);
      const bool pass = r >= f.range_min && (!f.filter_moving || s < 100u) && (!f.filter_outlier || s != 1u);
      if (pass) {
        cls[k] = lut[s];
        n_unknown += cls[k] < 0 ? 1 : 0;
      }
      keep[k] = pass && x[k] >= -f.radius && x[k] <= f.radius && y[k] >= -f.radius && y[k] <= f.radius && z[k] >= f.min_z &&
                z[k] <= f.max_z;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n_unknown += __shfl_xor(n_unknown, o, 64);
  if ((threadIdx.x & 63) == 0 && n_unknown > 0) atomicAdd(unknown, (unsigned long long)n_unknown);
  const int count = tile_ranks<FI>(sm, keep, rank);
  const long long excl = tile_exclusive_prefix(sm, state, tile, count);
#pragma unroll
  for (int k = 0; k < FI; ++k)
    if (keep[k]) {
      double* o = out + (excl + rank[k]) * 3;
      o[0] = x[k];
      o[1] = y[k];
      o[2] = z[k];
      class_out[excl + rank[k]] = cls[k];
    }
  if (tile == n_tiles - 1 && threadIdx.x == 0) *total = excl + count;
}

// ---- shine_depth_unproject -----------------------------------------------------------------------------------------------------
// Lane-major sibling of tile_ranks: element thread * ITEMS + k of a tile of ITEMS * T elements (every lane owns ITEMS CONSECUTIVE
// elements, so that it can fetch them in one vector load).  rank[k] = kept elements of the tile in front of that element (input
// order); returns the tile's kept count.
template <int ITEMS>
__device__ __forceinline__ int tile_ranks_lane_major(TileShared& sm, const bool (&keep)[ITEMS], int (&rank)[ITEMS]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  int in_front = 0, wave_total = 0;  // kept elements of the lanes below this one / of the whole wave
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const unsigned long long bal = __ballot(keep[k]);
    in_front += __popcll(bal & below);
    wave_total += __popcll(bal);
  }
  if (lane == 0) sm.cnt[wv] = wave_total;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int e = 0; e < T / 64; ++e) {
      sm.off[e] = run;
      run += sm.cnt[e];
    }
    sm.off[T / 64] = run;
  }
  __syncthreads();
  int own = sm.off[wv] + in_front;
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    rank[k] = own;
    own += keep[k] ? 1 : 0;
  }
  return sm.off[T / 64];
}

constexpr int DV = 4;  // pixels per lane, one 8-byte (uint16) or 16-byte (float32) load: a 640 x 480 image is 300 tiles of 1024

struct Unproject {
  double fx, fy, cx, cy;
  float depth_scale, depth_trunc;
  double m[12];  // cam_to_sensor, rows 0-2
  FilterBox box;
};

template <typename P>
struct PixelVec;
template <>
struct PixelVec<unsigned short> {
  typedef ushort4 type;
};
template <>
struct PixelVec<float> {
  typedef float4 type;
};

// One tile = DV * T consecutive pixels in row-major order (pixel i = row i / width, column i % width, at depth[row * pitch +
// column]).  A lane whose DV pixels lie in one row at an address aligned to the vector takes them in one load; every other lane
// (row ends, an unaligned base or pitch, the image's tail) takes them one by one.
template <typename P>
__global__ __launch_bounds__(T) void k_depth_unproject(const P* __restrict__ depth, int width, long long pitch, long long n,
                                                       Unproject q, double* __restrict__ out, int* __restrict__ index_out,
                                                       unsigned long long* state, unsigned int* counter, long long* total,
                                                       int n_tiles) {
#pragma clang fp contract(off)  // (every product and sum below is one correctly rounded IEEE operation, in the order written)
  typedef typename PixelVec<P>::type V;
  __shared__ TileShared sm;
  const int tile = take_ticket(sm, counter);
  const long long i0 = (long long)tile * (DV * T) + (long long)threadIdx.x * DV;
  P raw[DV];
  int col[DV], row[DV];
  bool keep[DV];
  int rank[DV];
  double x[DV], y[DV], z[DV];
#pragma unroll
  for (int k = 0; k < DV; ++k) {
    raw[k] = (P)0;
    col[k] = 0;
    row[k] = 0;
  }
  if (i0 < n) {
    const int r0 = (int)(i0 / width), c0 = (int)(i0 - (long long)r0 * width);
    const P* at = depth + (long long)r0 * pitch + c0;
    if (i0 + DV <= n && c0 + DV <= width && ((unsigned long long)at & (sizeof(V) - 1)) == 0) {
      const V v = *(const V*)at;
      raw[0] = v.x;
      raw[1] = v.y;
      raw[2] = v.z;
      raw[3] = v.w;
#pragma unroll
      for (int k = 0; k < DV; ++k) {
        row[k] = r0;
        col[k] = c0 + k;
      }
    } else {
#pragma unroll
      for (int k = 0; k < DV; ++k) {
        const long long i = i0 + k;
        if (i < n) {
          row[k] = (int)(i / width);
          col[k] = (int)(i - (long long)row[k] * width);
          raw[k] = depth[(long long)row[k] * pitch + col[k]];
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < DV; ++k) {
    const float d = __fdiv_rn((float)raw[k], q.depth_scale);
    keep[k] = false;
    // (a pixel past the image's end holds raw 0 and drops out here; NaN fails d > 0, +inf fails the last test)
    if (d > 0.0f && d < q.depth_trunc && d <= 3.402823466e+38f) {
      const double zc = (double)d;
      const double xc = ((double)col[k] - q.cx) * zc / q.fx;
      const double yc = ((double)row[k] - q.cy) * zc / q.fy;
      x[k] = q.m[0] * xc + q.m[1] * yc + q.m[2] * zc + q.m[3];
      y[k] = q.m[4] * xc + q.m[5] * yc + q.m[6] * zc + q.m[7];
      z[k] = q.m[8] * xc + q.m[9] * yc + q.m[10] * zc + q.m[11];
      const FilterBox& b = q.box;
      const double r = __dsqrt_rn(x[k] * x[k] + y[k] * y[k] + z[k] * z[k]);
      keep[k] = z[k] > b.min_z && r >= b.min_range && x[k] >= -b.radius && x[k] <= b.radius && y[k] >= -b.radius &&
                y[k] <= b.radius && z[k] >= b.min_z && z[k] <= b.max_z;
    }
  }
  const int count = tile_ranks_lane_major<DV>(sm, keep, rank);
  const long long excl = tile_exclusive_prefix(sm, state, tile, count);
#pragma unroll
  for (int k = 0; k < DV; ++k)
    if (keep[k]) {
      double* o = out + (excl + rank[k]) * 3;
      o[0] = x[k];
      o[1] = y[k];
      o[2] = z[k];
      if (index_out) index_out[excl + rank[k]] = (int)(i0 + k);
    }
  if (tile == n_tiles - 1 && threadIdx.x == 0) *total = excl + count;
}

// ---- shine_ray_sample ----------------------------------------------------------------------------------------------------------
// the sorted sampler's generator (shine_sampler_dev.hpp exp1v): splitmix64 finaliser of (seed, stream, counter), top 24 bits
__device__ __forceinline__ float uniform24(unsigned long long seed, unsigned long long stream, unsigned long long k) {
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (stream * 0x100000001B3ull + k + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (float)(unsigned int)(z >> 40) * (1.0f / 16777216.0f);  // [0, 1) on the 2^-24 grid
}

struct RayParams {
  float origin[3];
  int ns, nc, nf;
  float surface_range, clearance_dist, free_begin_ratio, free_end_dist, scale, time_value;
  unsigned long long seed, stream;
};

// One thread per OUTPUT sample t = ray * S + j: every per-sample array is written lane-contiguously.  The S threads of a ray
// each recompute its distance (three loads that hit the same cache lines, one sqrt) — cheaper than a second launch or an
// exchange.  fp32 in the reference's operation order, no contraction (utils/data_sampler.py:39-88).
__global__ __launch_bounds__(T) void k_ray_sample(const float* __restrict__ pts, long long m, RayParams p,
                                                  const int* __restrict__ labels, const float* __restrict__ uniforms,
                                                  float* __restrict__ coord, float* __restrict__ sdf_label,
                                                  float* __restrict__ weight, float* __restrict__ sample_depth,
                                                  int* __restrict__ sem_label, float* __restrict__ origin_out,
                                                  float* __restrict__ time_out, float* __restrict__ ray_depth) {
#pragma clang fp contract(off)
  __shared__ float s_xyz[3 * T];
  const int S = p.ns + p.nc + p.nf;
  const long long total = m * S;
  const long long base = (long long)blockIdx.x * T;
  const long long t = base + threadIdx.x;
  if (t < total) {
    const long long ray = t / S;
    const int j = (int)(t - ray * S);
    const float sx = pts[ray * 3] - p.origin[0], sy = pts[ray * 3 + 1] - p.origin[1], sz = pts[ray * 3 + 2] - p.origin[2];
    const float dist = sqrtf(sx * sx + sy * sy + sz * sz);
    // the reference's draw order: m * ns surface draws, then m * nc clearance, then m * nf free, each block sample-major
    long long u_at;
    int kind;  // 0 surface, 1 clearance, 2 free space
    if (j < p.ns) {
      kind = 0;
      u_at = (long long)j * m + ray;
    } else if (j < p.ns + p.nc) {
      kind = 1;
      u_at = m * p.ns + (long long)(j - p.ns) * m + ray;
    } else {
      kind = 2;
      u_at = m * (p.ns + p.nc) + (long long)(j - p.ns - p.nc) * m + ray;
    }
    const float u = uniforms ? uniforms[u_at] : uniform24(p.seed, p.stream, (unsigned long long)t);
    float disp, ratio;
    if (kind == 0) {
      disp = (u - 0.5f) * 2.0f * p.surface_range;
      ratio = disp / dist + 1.0f;
    } else if (kind == 1) {
      disp = -u * p.clearance_dist - p.surface_range;
      ratio = disp / dist + 1.0f;
    } else {
      const float hi = p.free_end_dist / dist + 1.0f;
      ratio = u * (hi - p.free_begin_ratio) + p.free_begin_ratio;
      disp = (ratio - 1.0f) * dist;
    }
    s_xyz[threadIdx.x * 3] = sx * ratio + p.origin[0];
    s_xyz[threadIdx.x * 3 + 1] = sy * ratio + p.origin[1];
    s_xyz[threadIdx.x * 3 + 2] = sz * ratio + p.origin[2];
    sdf_label[t] = disp;
    weight[t] = kind == 0 ? 1.0f : -1.0f;
    if (sample_depth) sample_depth[t] = dist * ratio / p.scale;
    if (sem_label) sem_label[t] = kind == 0 ? labels[ray] : 0;
    if (time_out) time_out[t] = p.time_value;
    if (ray_depth && j == 0) ray_depth[ray] = dist / p.scale;
  }
  __syncthreads();
  const long long rest = total - base;
  const int words = 3 * (int)(rest < T ? rest : T);
  for (int e = threadIdx.x; e < words; e += T) {  // base * 3 is a multiple of 3: word e of the block is axis e % 3
    coord[base * 3 + e] = s_xyz[e];
    if (origin_out) origin_out[base * 3 + e] = p.origin[e % 3];
  }
}

// ---- shine_pool_window_filter --------------------------------------------------------------------------------------------------
constexpr int WI = 4;
constexpr int MAX_ARRAYS = 6;

struct RowArrays {
  const unsigned int* src[MAX_ARRAYS];
  unsigned int* dst[MAX_ARRAYS];
  int words[MAX_ARRAYS];
  int n;
};

__global__ __launch_bounds__(T) void k_window_mask(const float* __restrict__ coord, long long n, float ox, float oy, float oz,
                                                   float radius, unsigned char* __restrict__ flags) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * T + threadIdx.x;
  if (i >= n) return;
  const float dx = coord[i * 3] - ox, dy = coord[i * 3 + 1] - oy, dz = coord[i * 3 + 2] - oz;
  flags[i] = sqrtf(dx * dx + dy * dy + dz * dz) < radius ? 1 : 0;
}

__global__ __launch_bounds__(T) void k_window_compact(const unsigned char* __restrict__ flags, long long n, RowArrays a,
                                                      unsigned long long* state, unsigned int* counter, long long* total,
                                                      int n_tiles) {
  __shared__ TileShared sm;
  const int tile = take_ticket(sm, counter);
  const long long base = (long long)tile * (WI * T);
  bool keep[WI];
  int rank[WI];
#pragma unroll
  for (int k = 0; k < WI; ++k) {
    const long long i = base + k * T + threadIdx.x;
    keep[k] = i < n && flags[i] != 0;
  }
  const int count = tile_ranks<WI>(sm, keep, rank);
  const long long excl = tile_exclusive_prefix(sm, state, tile, count);
#pragma unroll
  for (int k = 0; k < WI; ++k)
    if (keep[k]) {
      const long long i = base + k * T + threadIdx.x, o = excl + rank[k];
      for (int r = 0; r < a.n; ++r) {
        if (a.words[r] == 1) {
          a.dst[r][o] = a.src[r][i];
        } else {
          a.dst[r][o * 3] = a.src[r][i * 3];
          a.dst[r][o * 3 + 1] = a.src[r][i * 3 + 1];
          a.dst[r][o * 3 + 2] = a.src[r][i * 3 + 2];
        }
      }
    }
  if (tile == n_tiles - 1 && threadIdx.x == 0) *total = excl + count;
}

constexpr long long MAX_ROWS = (1ll << 31) - 1;  // (the tile ranks and the tile count are ints)

// the chained prefix's scratch: {counter, total, a second count} in one 256-byte slot, then one state word per tile
struct ChainScratch {
  unsigned int* counter;
  long long* total;
  unsigned long long* extra;  // (shine_sem_frame_filter's unknown-id count: bytes 16..23, next to total so that one copy fetches both)
  unsigned long long* state;
  size_t clear_bytes;
};
ChainScratch carve_chain(Arena& c, long long n_tiles) {
  ChainScratch s;
  const size_t before = c.bytes();
  unsigned long long* head = c.take<unsigned long long>(3);  // counter | total | extra, 8 bytes each
  s.counter = reinterpret_cast<unsigned int*>(head);
  s.total = reinterpret_cast<long long*>(head ? head + 1 : nullptr);
  s.extra = head ? head + 2 : nullptr;
  s.state = c.take<unsigned long long>((size_t)(n_tiles > 0 ? n_tiles : 1));
  s.clear_bytes = c.bytes() - before;
  return s;
}

}  // namespace
}  // namespace shine

using namespace shine;

extern "C" int shine_frame_filter(const void* points, int64_t n, int32_t is_fp64, int32_t stride, double min_z, double max_z,
                                  double min_range, double pc_radius, void* workspace, size_t* workspace_bytes,
                                  double* points_out, int64_t* n_out, void* stream) {
  if (!workspace_bytes || n < 0 || n > MAX_ROWS)
    return set_error(SHINE_E_INVALID, "shine_frame_filter: bad size (0 <= n < 2^31, workspace_bytes required)");
  if (stride != 3 && stride != 4) return set_error(SHINE_E_INVALID, "shine_frame_filter: stride must be 3 or 4 elements per point");
  const long long n_tiles = (n + FI * T - 1) / (FI * T);
  Arena c(workspace);
  ChainScratch s = carve_chain(c, n_tiles);
  SHINE_WORKSPACE_GATE(c.bytes(), workspace, workspace_bytes, "shine_frame_filter");
  if (!n_out) return set_error(SHINE_E_INVALID, "shine_frame_filter: null n_out");
  if (!(pc_radius >= 0.0) || !(max_z >= min_z) || min_range != min_range)
    return set_error(SHINE_E_INVALID, "shine_frame_filter: pc_radius < 0, max_z < min_z or a NaN bound");
  *n_out = 0;
  if (n == 0) return SHINE_OK;
  if (!points || !points_out) return set_error(SHINE_E_INVALID, "shine_frame_filter: null points");
  hipStream_t st = (hipStream_t)stream;
  SHINE_HIP_CHECK(hipMemsetAsync(s.counter, 0, s.clear_bytes, st));
  const FilterBox b{min_z, max_z, min_range, pc_radius};
  if (is_fp64)
    hipLaunchKernelGGL(k_frame_filter<double>, dim3((unsigned)n_tiles), dim3(T), 0, st, (const double*)points, (int)stride,
                       (long long)n, b, points_out, s.state, s.counter, s.total, (int)n_tiles);
  else
    hipLaunchKernelGGL(k_frame_filter<float>, dim3((unsigned)n_tiles), dim3(T), 0, st, (const float*)points, (int)stride,
                       (long long)n, b, points_out, s.state, s.counter, s.total, (int)n_tiles);
  SHINE_HIP_CHECK(hipGetLastError());
  long long total = 0;
  SHINE_HIP_CHECK(hipMemcpyAsync(&total, s.total, 8, hipMemcpyDeviceToHost, st));
  SHINE_HIP_CHECK(hipStreamSynchronize(st));
  *n_out = total;
  return SHINE_OK;
}

extern "C" int shine_sem_frame_filter(const void* points, int64_t n, int32_t is_fp64, int32_t stride, const uint32_t* labels,
                                      const int32_t* lut, double range_min, int32_t filter_moving, int32_t filter_outlier,
                                      double min_z, double max_z, double pc_radius, void* workspace, size_t* workspace_bytes,
                                      double* points_out, int32_t* class_out, int64_t* n_out, int64_t* n_unknown_out,
                                      void* stream) {
  if (!workspace_bytes || n < 0 || n > MAX_ROWS)
    return set_error(SHINE_E_INVALID, "shine_sem_frame_filter: bad size (0 <= n < 2^31, workspace_bytes required)");
  if (stride != 3 && stride != 4)
    return set_error(SHINE_E_INVALID, "shine_sem_frame_filter: stride must be 3 or 4 elements per point");
  const long long n_tiles = (n + FI * T - 1) / (FI * T);
  Arena c(workspace);
  ChainScratch s = carve_chain(c, n_tiles);
  SHINE_WORKSPACE_GATE(c.bytes(), workspace, workspace_bytes, "shine_sem_frame_filter");
  if (!n_out || !n_unknown_out) return set_error(SHINE_E_INVALID, "shine_sem_frame_filter: null n_out or n_unknown_out");
  if (!(pc_radius >= 0.0) || !(max_z >= min_z) || range_min != range_min)
    return set_error(SHINE_E_INVALID, "shine_sem_frame_filter: pc_radius < 0, max_z < min_z or a NaN bound");
  *n_out = 0;
  *n_unknown_out = 0;
  if (n == 0) return SHINE_OK;
  if (!points || !labels || !lut || !points_out || !class_out)
    return set_error(SHINE_E_INVALID, "shine_sem_frame_filter: null points, labels, lut, points_out or class_out");
  hipStream_t st = (hipStream_t)stream;
  SHINE_HIP_CHECK(hipMemsetAsync(s.counter, 0, s.clear_bytes, st));
  const SemFilter f{range_min, min_z, max_z, pc_radius, filter_moving != 0, filter_outlier != 0};
  if (is_fp64)
    hipLaunchKernelGGL(k_sem_frame_filter<double>, dim3((unsigned)n_tiles), dim3(T), 0, st, (const double*)points, (int)stride,
                       (const unsigned int*)labels, (const int*)lut, (long long)n, f, points_out, (int*)class_out, s.state,
                       s.counter, s.total, s.extra, (int)n_tiles);
  else
    hipLaunchKernelGGL(k_sem_frame_filter<float>, dim3((unsigned)n_tiles), dim3(T), 0, st, (const float*)points, (int)stride,
                       (const unsigned int*)labels, (const int*)lut, (long long)n, f, points_out, (int*)class_out, s.state,
                       s.counter, s.total, s.extra, (int)n_tiles);
  SHINE_HIP_CHECK(hipGetLastError());
  long long both[2] = {0, 0};  // {total, unknown}
  SHINE_HIP_CHECK(hipMemcpyAsync(both, s.total, 16, hipMemcpyDeviceToHost, st));
  SHINE_HIP_CHECK(hipStreamSynchronize(st));
  *n_out = both[0];
  *n_unknown_out = both[1];
  return SHINE_OK;
}

extern "C" int shine_depth_unproject(const void* depth, int32_t is_float32, int32_t width, int32_t height, int64_t row_pitch,
                                     double fx, double fy, double cx, double cy, double depth_scale, double depth_trunc,
                                     const double* cam_to_sensor, double min_z, double max_z, double min_range, double pc_radius,
                                     void* workspace, size_t* workspace_bytes, double* points_out, int32_t* index_out,
                                     int64_t* n_out, void* stream) {
  if (!workspace_bytes || width < 0 || height < 0 || (long long)width * height > MAX_ROWS)
    return set_error(SHINE_E_INVALID, "shine_depth_unproject: bad size (width, height >= 0, width * height < 2^31, workspace_bytes required)");
  if (row_pitch < width) return set_error(SHINE_E_INVALID, "shine_depth_unproject: row_pitch must be >= width (in pixels)");
  const long long n = (long long)width * height;
  const long long n_tiles = (n + DV * T - 1) / (DV * T);
  Arena c(workspace);
  ChainScratch s = carve_chain(c, n_tiles);
  SHINE_WORKSPACE_GATE(c.bytes(), workspace, workspace_bytes, "shine_depth_unproject");
  if (!n_out) return set_error(SHINE_E_INVALID, "shine_depth_unproject: null n_out");
  if (!(fx != 0.0) || !(fy != 0.0) || fx != fx || fy != fy || cx != cx || cy != cy)
    return set_error(SHINE_E_INVALID, "shine_depth_unproject: fx and fy must be non-zero, no NaN intrinsics");
  if (!(depth_scale > 0.0) || depth_trunc != depth_trunc)
    return set_error(SHINE_E_INVALID, "shine_depth_unproject: depth_scale must be > 0, depth_trunc not NaN");
  if (!(pc_radius >= 0.0) || !(max_z >= min_z) || min_range != min_range)
    return set_error(SHINE_E_INVALID, "shine_depth_unproject: pc_radius < 0, max_z < min_z or a NaN bound");
  *n_out = 0;
  if (n == 0) return SHINE_OK;
  if (!depth || !points_out) return set_error(SHINE_E_INVALID, "shine_depth_unproject: null depth or points_out");
  Unproject q;
  q.fx = fx;
  q.fy = fy;
  q.cx = cx;
  q.cy = cy;
  q.depth_scale = (float)depth_scale;
  q.depth_trunc = (float)depth_trunc;
  for (int e = 0; e < 12; ++e) q.m[e] = cam_to_sensor ? cam_to_sensor[e] : (e % 5 == 0 ? 1.0 : 0.0);
  q.box = FilterBox{min_z, max_z, min_range, pc_radius};
  hipStream_t st = (hipStream_t)stream;
  SHINE_HIP_CHECK(hipMemsetAsync(s.counter, 0, s.clear_bytes, st));
  if (is_float32)
    hipLaunchKernelGGL(k_depth_unproject<float>, dim3((unsigned)n_tiles), dim3(T), 0, st, (const float*)depth, (int)width,
                       (long long)row_pitch, n, q, points_out, (int*)index_out, s.state, s.counter, s.total, (int)n_tiles);
  else
    hipLaunchKernelGGL(k_depth_unproject<unsigned short>, dim3((unsigned)n_tiles), dim3(T), 0, st, (const unsigned short*)depth,
                       (int)width, (long long)row_pitch, n, q, points_out, (int*)index_out, s.state, s.counter, s.total,
                       (int)n_tiles);
  SHINE_HIP_CHECK(hipGetLastError());
  long long total = 0;
  SHINE_HIP_CHECK(hipMemcpyAsync(&total, s.total, 8, hipMemcpyDeviceToHost, st));
  SHINE_HIP_CHECK(hipStreamSynchronize(st));
  *n_out = total;
  return SHINE_OK;
}

extern "C" int shine_ray_sample(const float* points, int64_t m, const float* origin, int32_t surface_n, int32_t clearance_n,
                                int32_t free_n, float surface_range, float clearance_dist, float free_begin_ratio,
                                float free_end_dist, float scale, const int32_t* labels, uint64_t seed, uint64_t stream_id,
                                const float* uniforms, float time_value, float* coord_out, float* sdf_label_out,
                                float* weight_out, float* sample_depth_out, int32_t* sem_label_out, float* origin_out,
                                float* time_out, float* ray_depth_out, void* stream) {
  if (m < 0 || surface_n < 0 || clearance_n < 0 || free_n < 0)
    return set_error(SHINE_E_INVALID, "shine_ray_sample: negative ray or sample count");
  const long long S = (long long)surface_n + clearance_n + free_n;
  if (S == 0) return set_error(SHINE_E_INVALID, "shine_ray_sample: surface_n + clearance_n + free_n is zero");
  if (S > 4096 || m > MAX_ROWS / S) return set_error(SHINE_E_INVALID, "shine_ray_sample: m * S must be < 2^31");
  if (!origin) return set_error(SHINE_E_INVALID, "shine_ray_sample: null origin");
  if (!(scale > 0.0f)) return set_error(SHINE_E_INVALID, "shine_ray_sample: scale must be > 0");
  if (m == 0) return SHINE_OK;  // empty outputs, nothing launched
  if (!points || !coord_out || !sdf_label_out || !weight_out)
    return set_error(SHINE_E_INVALID, "shine_ray_sample: null points, coord_out, sdf_label_out or weight_out");
  if (sem_label_out && !labels) return set_error(SHINE_E_INVALID, "shine_ray_sample: sem_label_out needs labels");
  RayParams p;
  p.origin[0] = origin[0];
  p.origin[1] = origin[1];
  p.origin[2] = origin[2];
  p.ns = surface_n;
  p.nc = clearance_n;
  p.nf = free_n;
  p.surface_range = surface_range;
  p.clearance_dist = clearance_dist;
  p.free_begin_ratio = free_begin_ratio;
  p.free_end_dist = free_end_dist;
  p.scale = scale;
  p.time_value = time_value;
  p.seed = seed;
  p.stream = stream_id;
  const long long total = m * S;
  hipLaunchKernelGGL(k_ray_sample, dim3((unsigned)((total + T - 1) / T)), dim3(T), 0, (hipStream_t)stream, points, (long long)m, p,
                     labels, uniforms, coord_out, sdf_label_out, weight_out, sample_depth_out, sem_label_out, origin_out,
                     time_out, ray_depth_out);
  SHINE_HIP_CHECK(hipGetLastError());
  return SHINE_OK;
}

extern "C" int shine_pool_window_filter(const float* coord, int64_t n, const float* origin, float radius, int32_t n_arrays,
                                        const void* const* src, void* const* dst, const int32_t* words, void* workspace,
                                        size_t* workspace_bytes, int64_t* n_out, void* stream) {
  if (!workspace_bytes || n < 0 || n > MAX_ROWS)
    return set_error(SHINE_E_INVALID, "shine_pool_window_filter: bad size (0 <= n < 2^31, workspace_bytes required)");
  const long long n_tiles = (n + WI * T - 1) / (WI * T);
  Arena c(workspace);
  ChainScratch s = carve_chain(c, n_tiles);
  unsigned char* flags = c.take<unsigned char>((size_t)(n > 0 ? n : 1));
  SHINE_WORKSPACE_GATE(c.bytes(), workspace, workspace_bytes, "shine_pool_window_filter");
  if (!n_out || !origin) return set_error(SHINE_E_INVALID, "shine_pool_window_filter: null n_out or origin");
  if (!(radius > 0.0f)) return set_error(SHINE_E_INVALID, "shine_pool_window_filter: radius must be > 0");
  if (n_arrays < 1 || n_arrays > MAX_ARRAYS || !src || !dst || !words)
    return set_error(SHINE_E_INVALID, "shine_pool_window_filter: 1..6 arrays with src, dst and words");
  RowArrays a;
  a.n = n_arrays;
  for (int r = 0; r < n_arrays; ++r) {
    if (words[r] != 1 && words[r] != 3) return set_error(SHINE_E_INVALID, "shine_pool_window_filter: rows are 1 or 3 words");
    if (n > 0 && (!src[r] || !dst[r] || src[r] == dst[r]))
      return set_error(SHINE_E_INVALID, "shine_pool_window_filter: null array, or dst == src (not in place)");
    a.src[r] = (const unsigned int*)src[r];
    a.dst[r] = (unsigned int*)dst[r];
    a.words[r] = words[r];
  }
  *n_out = 0;
  if (n == 0) return SHINE_OK;
  if (!coord) return set_error(SHINE_E_INVALID, "shine_pool_window_filter: null coord");
  hipStream_t st = (hipStream_t)stream;
  SHINE_HIP_CHECK(hipMemsetAsync(s.counter, 0, s.clear_bytes, st));
  hipLaunchKernelGGL(k_window_mask, dim3((unsigned)((n + T - 1) / T)), dim3(T), 0, st, coord, (long long)n, origin[0], origin[1],
                     origin[2], radius, flags);
  SHINE_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_window_compact, dim3((unsigned)n_tiles), dim3(T), 0, st, (const unsigned char*)flags, (long long)n, a,
                     s.state, s.counter, s.total, (int)n_tiles);
  SHINE_HIP_CHECK(hipGetLastError());
  long long total = 0;
  SHINE_HIP_CHECK(hipMemcpyAsync(&total, s.total, 8, hipMemcpyDeviceToHost, st));
  SHINE_HIP_CHECK(hipStreamSynchronize(st));
  *n_out = total;
  return SHINE_OK;
}
