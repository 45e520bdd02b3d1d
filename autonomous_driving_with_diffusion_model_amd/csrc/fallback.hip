// Stop-short fallback (include/adx.h: adx_stop_short, "stop-short fallback v1"): re-time a plan so that it brakes to a halt before
// its first conflicting waypoint, for all rows of a tick in one launch.  No reference counterpart.
//
// One wave per row, four rows per workgroup, lane = waypoint; the waves of a workgroup share nothing (no LDS, no atomics, no
// barrier), so a row's result cannot depend on which rows share its launch.  Shaped like guide_cost_kernel (sched.hip) and
// control_step_kernel (control.hip):
//   1. lane h holds p_h and asks guide_grad (guide.h, as it is, under the scene view of its row) whether it conflicts; `first` is
//      one ballot and a find-first-set;
//   2. a free row is copied (a wave-uniform branch) and the wave leaves;
//   3. lane h takes seg_h from its neighbour's waypoint (one shuffle up); the arc lengths s_h are summed in index order: H - 1
//      trips, each a broadcast of lane h's seg, every lane advancing the same scalar and lane h keeping its s_h;
//   4. the speed profile q_h runs the same way: H - 1 trips of a dependent chain with one square root each -- the price of the
//      contract being sequential (profiles/README.md, "Stop-short fallback", has what it costs);
//   5. each lane looks its q_h up among s_0 .. s_{first-1} (a loop of `first` broadcasts, wave-uniform), fetches p_j and p_{j+1}
//      by indexed shuffles with all 64 lanes alive, and interpolates;
//   6. the residual is guide_grad on the output and the xor butterfly of adx_guide_cost; lane 0 stores the row's scalars with
//      plain vector stores.
// Lanes h >= H stay to the end, hold zeros and touch no memory.  Every product, sum, division and square root is rounded on its
// own (no contraction), so the bits do not depend on what the compiler would fuse.
#include "sched.h"

#pragma clang fp contract(off)      // the whole file: the contract's arithmetic

namespace adx {

namespace {

constexpr int kStopWaves = 4;

struct StopArgs {
  const float* traj;
  GuideArgs g;
  const float* params;
  float* out;
  int32_t* first;
  int32_t* status;
  float* stop_at;
  int32_t* active_after;
  int rows, horizon, dim, param_rows;
};

// The active count of waypoint (x, y) at index `h` of row `r`: what guide_cost_kernel<false> counts
__device__ __forceinline__ int waypoint_active(const GuideArgs& g, int r, int h, float x, float y) {
  float J, gx, gy;
  int active;
  guide_grad(scene_guide<true>(g, r), (float)h, x, y, J, gx, gy, active);
  return active;
}

__global__ void __launch_bounds__(kStopWaves* kWave) stop_short_kernel(const StopArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int r = blockIdx.x * kStopWaves + (threadIdx.x >> 6);
  if (r >= a.rows) return;                       // whole waves leave: the shuffles below always see all 64 lanes
  const int H = a.horizon, D = a.dim;
  const bool live = lane < H;
  const float* src = a.traj + ((size_t)r * H + lane) * D;
  float* dst = a.out + ((size_t)r * H + lane) * D;
  const bool copy = a.out != a.traj;             // in place: what is not re-timed is already there

  // 1. conflicts
  float x = 0.f, y = 0.f;
  bool conflict = false;
  if (live) {
    x = src[0]; y = src[1];
    conflict = waypoint_active(a.g, r, lane, x, y) > 0 || !finite_f(x) || !finite_f(y);
  }
  const unsigned long long hits = __ballot(conflict);
  const int first = hits != 0ull ? __ffsll(hits) - 1 : H;

  // 2. a free row
  if (first == H) {
    if (live && copy) {
      for (int d = 0; d < D; ++d) dst[d] = src[d];
    }
    if (lane == 0) {
      a.first[r] = first;
      a.status[r] = 0;
      a.stop_at[r] = __builtin_inff();
      a.active_after[r] = 0;
    }
    return;
  }

  // 3. arc length, in index order
  const float px = __shfl_up(x, 1, kWave), py = __shfl_up(y, 1, kWave);
  float seg = 0.f;
  if (lane >= 1 && lane < first) {
    const float dx = x - px, dy = y - py;
    seg = sqrtf(dx * dx + dy * dy);
  }
  float run = 0.f, s_h = 0.f;
  for (int i = 1; i < H; ++i) {
    run = run + __shfl(seg, i, kWave);
    if (lane == i) s_h = run;
  }

  // 4. the stop point and the speed profile
  const float* prm = a.params + (size_t)(r % a.param_rows) * 2;
  const float gap = prm[0], decel = prm[1];
  const float g = gap >= 0.f ? gap : 0.f;
  float L = 0.f;
  if (first >= 1) {
    const float t = __shfl(s_h, first - 1, kWave) - g;
    L = t > 0.f ? t : 0.f;
  }
  const bool limited = finite_f(decel) && decel >= 0.f;
  const float aa = decel * decel, a8 = 8.0f * decel;
  float q = 0.f, q_h = 0.f, u1 = 0.f;
  for (int i = 1; i < H; ++i) {
    const float d = L - q;
    const float w = i < first ? __shfl(seg, i, kWave) : __builtin_inff();
    float u = d < w ? d : w;
    if (limited) {
      const float ad = a8 * d;
      const float e = (sqrtf(aa + ad) - decel) * 0.5f;
      u = e < u ? e : u;
    }
    q = q + u;
    if (lane == i) q_h = q;
    if (i == 1) u1 = u;
  }
  const float seg1 = __shfl(seg, 1, kWave);
  const int status = (H > 1 && first > 1 && limited && seg1 - u1 > decel) ? 2 : 1;

  // 5. resample: the largest j in 0 .. first - 1 with s_j <= q_h, then along segment j
  int j = 0;
  float s_j = 0.f;
  for (int k = 0; k < first; ++k) {
    const float s_k = __shfl(s_h, k, kWave);
    if (s_k <= q_h) { j = k; s_j = s_k; }
  }
  const int jn = (j + 1) & (kWave - 1);
  const float jx = __shfl(x, j, kWave), jy = __shfl(y, j, kWave);
  const float nx = __shfl(x, jn, kWave), ny = __shfl(y, jn, kWave);
  const float s_n = __shfl(s_h, jn, kWave);
  float ox = jx, oy = jy;                        // first == 0: j = 0, p_0
  if (first != 0 && j != first - 1 && !(q_h == s_j)) {
    const float t = (q_h - s_j) / (s_n - s_j);
    ox = jx + t * (nx - jx);
    oy = jy + t * (ny - jy);
  }

  // 6. the residual, and the stores
  int active = 0;
  if (live) {
    active = waypoint_active(a.g, r, lane, ox, oy);
    dst[0] = ox; dst[1] = oy;
    if (copy) {
      for (int d = 2; d < D; ++d) dst[d] = src[d];
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) active += __shfl_xor(active, off, kWave);
  if (lane == 0) {
    a.first[r] = first;
    a.status[r] = status;
    a.stop_at[r] = L;
    a.active_after[r] = active;
  }
}

}  // namespace

int stop_short(const float* traj, const GuideRecords& g, const float* params, int param_rows, float* out, int32_t* first,
               int32_t* status, float* stop_at, int32_t* active_after, int rows, int horizon, int dim, hipStream_t s) {
  const char* const what = "stop short";
  ADX_REQUIRE(traj != nullptr && out != nullptr && params != nullptr && first != nullptr && status != nullptr && stop_at != nullptr &&
                  active_after != nullptr, "stop short: null traj, out, params, first, status, stop_at or active_after");
  ADX_REQUIRE(g.guide != nullptr || g.field != nullptr, "stop short: null guide and null field");
  ADX_REQUIRE(horizon >= 1 && horizon <= kWave, "stop short: horizon %d outside 1..%d", horizon, kWave);
  ADX_REQUIRE(dim >= 2, "stop short: the fallback re-times (x, y), dim is %d", dim);
  ADX_REQUIRE(param_rows >= 1, "stop short: param_rows %d, at least 1", param_rows);
  int rc = shape_check(what, rows, horizon, dim);      // horizon and dim are in range by now: what is left is `rows`
  if (rc != ADX_OK) return rc;
  StopArgs a;
  const size_t tn = (size_t)rows * horizon * dim * sizeof(float), cn = (size_t)rows * sizeof(float);
  const size_t pn = (size_t)param_rows * 2 * sizeof(float);
  const ByteSpan outs[5] = {{out, tn}, {first, cn}, {status, cn}, {stop_at, cn}, {active_after, cn}};
  // no MotionArgs: the limits couple waypoints, the fallback asks about one waypoint at a time, so g.motion is neither checked nor read
  rc = guide_records_check(g, what, false, false, outs, 5, rows, horizon, dim, &a.g, nullptr);
  if (rc != ADX_OK) return rc;
  ADX_REQUIRE(a.g.M > 0 || a.g.P > 0 || a.g.field.cells != nullptr || a.g.route.points != nullptr || a.g.capsule.slots != nullptr,
              "stop short: the guide holds no point-wise term (discs, planes, a field, a route or capsules)");
  for (int i = 0; i < 5; ++i) {
    bool bad = byte_ranges_overlap(outs[i].p, outs[i].n, params, pn) ||
               (!(i == 0 && out == traj) && byte_ranges_overlap(outs[i].p, outs[i].n, traj, tn));
    for (int k = i + 1; k < 5; ++k) bad = bad || byte_ranges_overlap(outs[i].p, outs[i].n, outs[k].p, outs[k].n);
    ADX_REQUIRE(!bad, "stop short: an output overlaps traj, params or another output (out == traj, the same pointer, is allowed)");
  }
  a.traj = traj; a.params = params; a.out = out; a.first = first; a.status = status; a.stop_at = stop_at;
  a.active_after = active_after; a.rows = rows; a.horizon = horizon; a.dim = dim; a.param_rows = param_rows;
  stop_short_kernel<<<dim3(ceil_div(rows, kStopWaves)), dim3(kStopWaves * kWave), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

}  // namespace adx
