// Best-of-K trajectory selection (include/adx.h: adx_traj_select, "selection cost v1").  No reference counterpart: the
// reference's train.evaluate draws many trajectories for one image only to paint them (train.py:62-90).
//
// One workgroup per scene, 256 threads = 4 waves.  The scene's K x H xy pairs are staged in LDS as two planes (x, y), so that
// every later read is a 4-byte read at consecutive lanes = consecutive banks (conflict-free in both 32-lane halves, the h - 1
// and h + 1 neighbours of the smoothness term included).  Then
//   1. the mean path: wave w adds candidates k = w, w + 4, ... in that order (lane = waypoint), the four partial sums meet in
//      LDS and are added as (p0 + p1) + (p2 + p3);
//   2. the costs: wave w walks the same candidates with lane = waypoint and reduces the three terms over the wave with xor
//      butterflies (every lane ends with the same value; the tree does not depend on K or on the launch);
//   3. the first wave's arg-min over the K costs (lane = candidate), ties and non-finite costs by the rule of the contract;
//   4. all threads copy the winning row word for word.
// No atomics and no inter-workgroup traffic: a given input gives the same bits on every launch.  Every product and sum is
// rounded on its own (no contraction), so the bits do not depend on what the compiler would fuse either.
#include "adx_common.h"

namespace adx {

namespace {

constexpr int kSelMaxK = 64, kSelMaxH = 64, kSelMaxD = 16, kSelWaves = 4;

struct SelectArgs {
  const float* trajs;
  const float* target;   // [scenes][2] or null
  float* cost;
  int32_t* index;
  float* best;
  int scenes, K, H, D;
  float w_goal, w_smooth, w_consensus;
};

// minimum that a NaN wins (numpy's min): the goal term of a candidate with a NaN waypoint is NaN
__device__ __forceinline__ float min_nan(float a, float b) { return (a != a) ? a : ((b != b) ? b : fminf(a, b)); }

__device__ __forceinline__ float wave_min_nan(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min_nan(v, __shfl_xor(v, off, 64));
  return v;
}

__global__ void __launch_bounds__(256) traj_select_kernel(const SelectArgs a) {
#pragma clang fp contract(off)
  __shared__ float xs[kSelMaxK * kSelMaxH], ys[kSelMaxK * kSelMaxH];
  __shared__ float part_x[kSelWaves][kSelMaxH], part_y[kSelWaves][kSelMaxH];
  __shared__ float cost_s[kSelMaxK];
  __shared__ int win_s;
  const int s = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int K = a.K, H = a.H, D = a.D;
  const size_t row_floats = (size_t)H * D;

  // stage: element i = k * H + h of the scene; candidate k of scene s is row k * scenes + s
  for (int i = tid; i < K * H; i += 256) {
    const int k = i / H, h = i - k * H;
    const float* p = a.trajs + ((size_t)k * a.scenes + s) * row_floats + (size_t)h * D;
    xs[i] = p[0];
    ys[i] = D > 1 ? p[1] : 0.f;
  }
  __syncthreads();

  const bool live = lane < H;
  {  // 1. mean path
    float sx = 0.f, sy = 0.f;
    if (live)
      for (int k = wave; k < K; k += kSelWaves) { sx += xs[k * H + lane]; sy += ys[k * H + lane]; }
    part_x[wave][lane] = sx;
    part_y[wave][lane] = sy;
  }
  __syncthreads();
  float mx = 0.f, my = 0.f;
  if (live) {
    const float kf = (float)K;
    mx = ((part_x[0][lane] + part_x[1][lane]) + (part_x[2][lane] + part_x[3][lane])) / kf;
    my = ((part_y[0][lane] + part_y[1][lane]) + (part_y[2][lane] + part_y[3][lane])) / kf;
  }

  // 2. costs.  A term whose weight is exactly 0 is not evaluated (it contributes +0, whatever its value would be).
  const bool use_goal = a.target != nullptr && a.w_goal != 0.f;
  const bool use_smooth = a.w_smooth != 0.f && H >= 3;
  const bool use_cons = a.w_consensus != 0.f;
  float gx = 0.f, gy = 0.f;
  if (use_goal) { gx = a.target[2 * s]; gy = a.target[2 * s + 1]; }
  for (int k = wave; k < K; k += kSelWaves) {      // wave-uniform trip count: the shuffles below see all 64 lanes
    const int base = k * H;
    const float px = live ? xs[base + lane] : 0.f, py = live ? ys[base + lane] : 0.f;
    float cost = 0.f;
    if (use_goal) {
      const float dx = px - gx, dy = py - gy;
      const float d2 = dx * dx + dy * dy;
      const float goal = wave_min_nan(live ? d2 : __builtin_inff());
      cost = a.w_goal * goal;
    }
    if (use_smooth) {
      float t = 0.f;
      if (lane >= 1 && lane <= H - 2) {
        const float ax = (xs[base + lane + 1] - 2.f * px) + xs[base + lane - 1];
        const float ay = (ys[base + lane + 1] - 2.f * py) + ys[base + lane - 1];
        t = ax * ax + ay * ay;
      }
      const float smooth = wave_sum(t) / (float)(H - 2);
      cost = cost + a.w_smooth * smooth;
    }
    if (use_cons) {
      float t = 0.f;
      if (live) {
        const float dx = px - mx, dy = py - my;
        t = dx * dx + dy * dy;
      }
      const float cons = wave_sum(t) / (float)H;
      cost = cost + a.w_consensus * cons;
    }
    if (lane == 0) {
      cost_s[k] = cost;
      a.cost[(size_t)s * K + k] = cost;
    }
  }
  __syncthreads();

  // 3. arg-min: the smallest k among the smallest finite costs; no finite cost at all -> every key is +inf -> k = 0
  if (wave == 0) {
    float v = __builtin_inff();
    int idx = lane;
    if (lane < K) {
      const float c = cost_s[lane];
      if (__builtin_fabsf(c) < __builtin_inff()) v = c;     // false for inf and NaN
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(v, off, 64);
      const int oi = __shfl_xor(idx, off, 64);
      if (ov < v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
    if (lane == 0) {
      win_s = idx;
      a.index[s] = idx;
    }
  }
  __syncthreads();

  // 4. the winner's full [H][D] row, bit for bit
  const int win = win_s;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.trajs + ((size_t)win * a.scenes + s) * row_floats);
  uint32_t* dst = reinterpret_cast<uint32_t*>(a.best + (size_t)s * row_floats);
  for (int i = tid; i < H * D; i += 256) dst[i] = src[i];
}

bool overlaps(const void* p, size_t pn, const void* q, size_t qn) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + qn && b < a + pn;
}

}  // namespace

int traj_select(const adx_select_cfg* c, const float* trajs, const float* target, float* cost, int32_t* index, float* best,
                hipStream_t s) {
  ADX_REQUIRE(c != nullptr, "traj select: null configuration");
  ADX_REQUIRE(c->candidates >= 1 && c->candidates <= kSelMaxK, "traj select: %d candidates, supported 1..%d", c->candidates, kSelMaxK);
  ADX_REQUIRE(c->horizon >= 1 && c->horizon <= kSelMaxH, "traj select: horizon %d, supported 1..%d", c->horizon, kSelMaxH);
  ADX_REQUIRE(c->dim >= 1 && c->dim <= kSelMaxD, "traj select: transition dim %d, supported 1..%d", c->dim, kSelMaxD);
  ADX_REQUIRE(c->scenes >= 1 && c->scenes <= 65535, "traj select: %d scenes, supported 1..65535", c->scenes);
  ADX_REQUIRE(trajs != nullptr && cost != nullptr && index != nullptr && best != nullptr, "traj select: null tensor");
  const size_t row = (size_t)c->horizon * c->dim * sizeof(float);
  const size_t in_bytes = (size_t)c->candidates * c->scenes * row, best_bytes = (size_t)c->scenes * row;
  const size_t cost_bytes = (size_t)c->scenes * c->candidates * sizeof(float), index_bytes = (size_t)c->scenes * sizeof(int32_t);
  ADX_REQUIRE(!overlaps(best, best_bytes, trajs, in_bytes) && !overlaps(cost, cost_bytes, trajs, in_bytes) &&
                  !overlaps(index, index_bytes, trajs, in_bytes),
              "traj select: an output aliases trajs");
  ADX_REQUIRE(!overlaps(best, best_bytes, cost, cost_bytes) && !overlaps(best, best_bytes, index, index_bytes) &&
                  !overlaps(cost, cost_bytes, index, index_bytes),
              "traj select: outputs alias each other");
  SelectArgs a;
  a.trajs = trajs; a.target = target; a.cost = cost; a.index = index; a.best = best;
  a.scenes = c->scenes; a.K = c->candidates; a.H = c->horizon; a.D = c->dim;
  a.w_goal = c->w_goal; a.w_smooth = c->w_smooth; a.w_consensus = c->w_consensus;
  traj_select_kernel<<<dim3(c->scenes), dim3(256), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

}  // namespace adx
