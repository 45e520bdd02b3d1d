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
//
// "Selection cost v2" (adx_traj_select_guide) is a second instantiation of the same kernel (kGuide): the scene's discs and planes
// are staged in LDS beside xs / ys (every lane of a wave reads the same constraint word: a broadcast, no bank conflict), step 2
// also evaluates each waypoint's "cost guidance v1" cost and active count with the routine the step kernels use (guide.h: the
// scene view of scene_guide, its discs and planes pointed at the LDS copies) from the LDS copy of xy, reduces them with the
// butterflies adx_guide_cost uses and takes a wave-wide vote on "every xy finite"; step 3 searches the free candidates alone when
// `hard` is set and one of them has a finite cost, and reports whether the winner is blocked.  The kGuide = false instantiation
// reads none of the fields behind w_consensus: its code is what it was.
// With a field ("cost guidance v2") the same routine also reads the scene's raster, from global memory: four cells per waypoint.
// With motion limits ("cost guidance v3", the kMotion instantiation) a waypoint's share of the segment and curvature terms follows,
// through guide.h's motion_grad; its four neighbours are read from the xy planes in LDS.
// With a route ("cost guidance v4") guide_grad also reads the scene's polyline, from global memory: no kernel variant, a uniform branch.
// With capsules ("cost guidance v5") it reads the scene's slots the same way.
#include "sched.h"

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
  // selection cost v2 (the kGuide kernel only)
  GuideArgs guide;
  float w_guide;
  int hard;
  int32_t* active;       // [scenes][K]
  int32_t* blocked;      // [scenes]
  MotionArgs motion;     // cost guidance v3 (the kMotion kernel only)
};

// minimum that a NaN wins (numpy's min): the goal term of a candidate with a NaN waypoint is NaN
__device__ __forceinline__ float min_nan(float a, float b) { return (a != a) ? a : ((b != b) ? b : fminf(a, b)); }

__device__ __forceinline__ float wave_min_nan(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min_nan(v, __shfl_xor(v, off, 64));
  return v;
}

template <bool kGuide, bool kMotion = false>
__global__ void __launch_bounds__(256) traj_select_kernel(const SelectArgs a) {
#pragma clang fp contract(off)
  __shared__ float xs[kSelMaxK * kSelMaxH], ys[kSelMaxK * kSelMaxH];
  __shared__ float part_x[kSelWaves][kSelMaxH], part_y[kSelWaves][kSelMaxH];
  __shared__ float cost_s[kSelMaxK];
  __shared__ int win_s;
  // kGuide only (an instantiation that never touches them allocates none of it): the scene's constraints and free[k]
  __shared__ float disc_s[ADX_GUIDE_MAX_DISCS * 5], plane_s[ADX_GUIDE_MAX_PLANES * 3];
  __shared__ int free_s[kSelMaxK];
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
  SceneGuide scene = {};
  if constexpr (kGuide) {      // the scene's discs and planes, once: the M * 5 and P * 3 words are within the arrays (the host checked)
    scene = scene_guide(a.guide, s);
    for (int i = tid; i < scene.M * 5; i += 256) disc_s[i] = scene.discs[i];
    for (int i = tid; i < scene.P * 3; i += 256) plane_s[i] = scene.planes[i];
    scene.discs = disc_s;      // from here on every lane of a wave reads the same constraint word of the LDS copy
    scene.planes = plane_s;
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
    if constexpr (kGuide) {
      // violation and active count exactly as guide_cost_kernel forms them: lane = waypoint, lanes h >= H hold 0, the same two
      // butterflies.  The count and the vote run whatever the weights; the weighted term only when asked for
      float J = 0.f;
      int act = 0;
      if (live) {
        float jx, jy;
        guide_grad(scene, (float)lane, px, py, J, jx, jy, act);      // the raster, the route and the capsules from global memory
        if constexpr (kMotion) {      // the neighbours from the planes; a point outside the row is a zero no term reads
          float nx[5], ny[5], S2, A2;
#pragma unroll
          for (int j = 0; j < 5; ++j) {
            const int h = lane - 2 + j;
            const bool in = h >= 0 && h < H;
            nx[j] = in ? xs[base + h] : 0.f;
            ny[j] = in ? ys[base + h] : 0.f;
          }
          motion_limits(a.motion, s, S2, A2);
          motion_grad(nx, ny, lane, H, S2, A2, a.motion.w_speed, a.motion.w_accel, J, jx, jy, act);
        }
      }
      if (a.w_guide != 0.f) {
        const float violation = wave_sum(J);
        cost = cost + a.w_guide * violation;
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) act += __shfl_xor(act, off, 64);
      // a NaN waypoint compares false against every constraint: it must not count as "violates nothing"
      const bool odd = live && !(__builtin_fabsf(px) < __builtin_inff() && __builtin_fabsf(py) < __builtin_inff());
      const bool all_finite = __ballot(odd) == 0ull;
      if (lane == 0) {
        a.active[(size_t)s * K + k] = act;
        free_s[k] = (act == 0 && all_finite) ? 1 : 0;
      }
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
    if constexpr (kGuide) {
      // the two-set rule: when some free candidate has a finite cost, the others' keys become +inf and the same search runs on
      // what is left (the winner then has a finite key, so a masked lane can never be picked by the tie rule)
      if (a.hard) {
        const bool free_finite = lane < K && free_s[lane] != 0 && v < __builtin_inff();
        if (__ballot(free_finite) != 0ull && !free_finite) v = __builtin_inff();
      }
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
      if constexpr (kGuide) a.blocked[s] = free_s[idx] != 0 ? 0 : 1;
    }
  }
  __syncthreads();

  // 4. the winner's full [H][D] row, bit for bit
  const int win = win_s;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.trajs + ((size_t)win * a.scenes + s) * row_floats);
  uint32_t* dst = reinterpret_cast<uint32_t*>(a.best + (size_t)s * row_floats);
  for (int i = tid; i < H * D; i += 256) dst[i] = src[i];
}

// the refusals of "selection cost v1", which v2 inherits: the limits, the pointers both versions have, their overlaps
int select_check(int scenes, int K, int H, int D, const float* trajs, const float* cost, const int32_t* index, const float* best) {
  ADX_REQUIRE(K >= 1 && K <= kSelMaxK, "traj select: %d candidates, supported 1..%d", K, kSelMaxK);
  ADX_REQUIRE(H >= 1 && H <= kSelMaxH, "traj select: horizon %d, supported 1..%d", H, kSelMaxH);
  ADX_REQUIRE(D >= 1 && D <= kSelMaxD, "traj select: transition dim %d, supported 1..%d", D, kSelMaxD);
  ADX_REQUIRE(scenes >= 1 && scenes <= 65535, "traj select: %d scenes, supported 1..65535", scenes);
  ADX_REQUIRE(trajs != nullptr && cost != nullptr && index != nullptr && best != nullptr, "traj select: null tensor");
  const size_t row = (size_t)H * D * sizeof(float);
  const size_t in_bytes = (size_t)K * scenes * row, best_bytes = (size_t)scenes * row;
  const size_t cost_bytes = (size_t)scenes * K * sizeof(float), index_bytes = (size_t)scenes * sizeof(int32_t);
  ADX_REQUIRE(!byte_ranges_overlap(best, best_bytes, trajs, in_bytes) && !byte_ranges_overlap(cost, cost_bytes, trajs, in_bytes) &&
                  !byte_ranges_overlap(index, index_bytes, trajs, in_bytes),
              "traj select: an output aliases trajs");
  ADX_REQUIRE(!byte_ranges_overlap(best, best_bytes, cost, cost_bytes) && !byte_ranges_overlap(best, best_bytes, index, index_bytes) &&
                  !byte_ranges_overlap(cost, cost_bytes, index, index_bytes),
              "traj select: outputs alias each other");
  return ADX_OK;
}

}  // namespace

int traj_select(const adx_select_cfg* c, const float* trajs, const float* target, float* cost, int32_t* index, float* best,
                hipStream_t s) {
  ADX_REQUIRE(c != nullptr, "traj select: null configuration");
  const int rc = select_check(c->scenes, c->candidates, c->horizon, c->dim, trajs, cost, index, best);
  if (rc != ADX_OK) return rc;
  SelectArgs a = {};
  a.trajs = trajs; a.target = target; a.cost = cost; a.index = index; a.best = best;
  a.scenes = c->scenes; a.K = c->candidates; a.H = c->horizon; a.D = c->dim;
  a.w_goal = c->w_goal; a.w_smooth = c->w_smooth; a.w_consensus = c->w_consensus;
  traj_select_kernel<false><<<dim3(c->scenes), dim3(256), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

// "Selection cost v2": v1's refusals first, then what the guide records ask of the five outputs (sched.h: with a field the guide
// may be null), then what is the selection's own: candidate k of scene s is row k * S + s, so only scene_rows == S makes
// row % scene_rows the scene; and the new outputs against trajs and against every other output
int traj_select_guide(const adx_select_guide_cfg* c, const float* trajs, const float* target, const GuideRecords& g, float* cost,
                      int32_t* active, int32_t* index, int32_t* blocked, float* best, hipStream_t s) {
  const char* const what = "traj select guide";
  ADX_REQUIRE(c != nullptr, "traj select: null configuration");
  int rc = select_check(c->scenes, c->candidates, c->horizon, c->dim, trajs, cost, index, best);
  if (rc != ADX_OK) return rc;
  ADX_REQUIRE(c->dim >= 2, "traj select guide: the guide scores (x, y), dim is %d", c->dim);
  ADX_REQUIRE(g.guide != nullptr || g.field != nullptr, "traj select guide: null guide");
  ADX_REQUIRE(active != nullptr, "traj select guide: null active");
  ADX_REQUIRE(blocked != nullptr, "traj select guide: null blocked");
  const int S = c->scenes, K = c->candidates;
  const size_t row = (size_t)c->horizon * c->dim * sizeof(float);
  const size_t in_bytes = (size_t)K * S * row, best_bytes = (size_t)S * row;
  const size_t sk_bytes = (size_t)S * K * sizeof(float), s_bytes = (size_t)S * sizeof(int32_t);
  SelectArgs a = {};
  const ByteSpan outs[5] = {{cost, sk_bytes}, {active, sk_bytes}, {index, s_bytes}, {blocked, s_bytes}, {best, best_bytes}};
  rc = guide_records_check(g, what, false, false, outs, 5, S * K, c->horizon, c->dim, &a.guide, &a.motion);
  if (rc != ADX_OK) return rc;
  if (g.guide != nullptr) {
    const bool bare = g.guide->n_discs == 0 && g.guide->n_planes == 0;
    ADX_REQUIRE(g.guide->scene_rows == S || (g.guide->scene_rows == 1 && bare),
                "traj select guide: the guide holds %d scenes, the selection %d (1 is accepted of a guide without discs and planes)",
                g.guide->scene_rows, S);
  }
  ADX_REQUIRE(g.field == nullptr || g.field->scene_rows == S, "traj select guide: the field holds %d scenes, the selection %d",
              g.field == nullptr ? 0 : g.field->scene_rows, S);
  ADX_REQUIRE(g.motion == nullptr || g.motion->scene_rows == S, "traj select guide: the limits hold %d scenes, the selection %d",
              g.motion == nullptr ? 0 : g.motion->scene_rows, S);
  ADX_REQUIRE(g.route == nullptr || g.route->scene_rows == S, "traj select guide: the route holds %d scenes, the selection %d",
              g.route == nullptr ? 0 : g.route->scene_rows, S);
  ADX_REQUIRE(g.capsules == nullptr || g.capsules->scene_rows == S, "traj select guide: the capsules hold %d scenes, the selection %d",
              g.capsules == nullptr ? 0 : g.capsules->scene_rows, S);
  ADX_REQUIRE(!byte_ranges_overlap(active, sk_bytes, trajs, in_bytes) && !byte_ranges_overlap(blocked, s_bytes, trajs, in_bytes),
              "traj select guide: an output aliases trajs");
  ADX_REQUIRE(!byte_ranges_overlap(active, sk_bytes, cost, sk_bytes) && !byte_ranges_overlap(active, sk_bytes, index, s_bytes) &&
                  !byte_ranges_overlap(active, sk_bytes, best, best_bytes) && !byte_ranges_overlap(active, sk_bytes, blocked, s_bytes) &&
                  !byte_ranges_overlap(blocked, s_bytes, cost, sk_bytes) && !byte_ranges_overlap(blocked, s_bytes, index, s_bytes) &&
                  !byte_ranges_overlap(blocked, s_bytes, best, best_bytes),
              "traj select guide: outputs alias each other");
  a.trajs = trajs; a.target = target; a.cost = cost; a.index = index; a.best = best;
  a.scenes = S; a.K = K; a.H = c->horizon; a.D = c->dim;
  a.w_goal = c->w_goal; a.w_smooth = c->w_smooth; a.w_consensus = c->w_consensus;
  a.w_guide = c->w_guide; a.hard = c->hard != 0; a.active = active; a.blocked = blocked;
  if (g.motion != nullptr) traj_select_kernel<true, true><<<dim3(S), dim3(256), 0, s>>>(a);
  else traj_select_kernel<true><<<dim3(S), dim3(256), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

}  // namespace adx
