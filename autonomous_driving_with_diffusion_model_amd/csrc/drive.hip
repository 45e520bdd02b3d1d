// What scores a drive (include/adx.h: "drive metrics v1"): route completion, cross-track error, collisions, route deviation, a stall
// clock, comfort and the odometer of every scene, advanced by one tick per launch with the records in device memory.
//
// fp64, no contraction, latency-bound like nav.hip, and laid out like it:
//   drive_step_kernel   one workgroup of one wave per scene.  The parallel part is the nearest point of the route -- a projection
//                       and a square root per segment -- and the obstacles: lanes take 64 segments at a time and one xor butterfly
//                       over (d, j) keeps the nearest, the lower index on a tie; lane j tests disc j and box j against the ego's
//                       discs and a ballot reduces the hit.  The record itself is sequential bookkeeping: lane 0 forms it in LDS,
//                       then lanes 0 .. 47 store one 32-bit word of it each (narrow stores, for nav.hip's reason).
//   drive_reset_kernel  one thread per word.
// No atomics, no traffic between workgroups: the same inputs and state give the same bits on every launch.
#include "sched.h"

#pragma clang fp contract(off)

namespace adx {

namespace {

constexpr int kDriveMaxScenes = 65535, kDriveMaxPoints = 65536, kDriveMaxSlots = 64, kDriveWords = 48;

struct DriveState {      // 192 bytes per scene; all zero = a drive not yet begun
  int32_t cursor, ticks, done, flags, contact, events, contact_ticks, first_tick, first_slot, have;
  double px, py, v_prev, a_prev, progress, progress_max, xtrack, xtrack_max, xtrack_sum, xtrack_sq, distance, offroad, stall, acc_max,
      acc_sq, jerk_max, jerk_sq, lat_max, lat_sq;
};
static_assert(sizeof(DriveState) == 4 * kDriveWords, "drive metrics v1: 192 bytes of state per scene");

__device__ __forceinline__ double norm2(double x, double y) {
  const double xx = x * x, yy = y * y;
  return sqrt(xx + yy);
}

__device__ __forceinline__ double max0(double v) { return v > 0.0 ? v : 0.0; }

struct DriveArgs {
  const double* pose;        // [S][3]
  const float* velocity;     // [S]
  const float* yaw_rate;     // [S]
  const double* route;       // [S][G][2]
  const int32_t* len;        // [S]
  const double* cum;         // [S][G]
  const double* discs;       // [S][M][5] or null
  const double* boxes;       // [S][N][7] or null
  DriveState* state;         // [S]
  int32_t* done;             // [S]
  int G, window, M, N, n_discs, stop_on_collision, max_ticks;
  double dt, r_ego, offset[4], offroad_min, offroad_max, share, speed_threshold, max_time, completion_tol;
};

__global__ void __launch_bounds__(64) drive_step_kernel(const DriveArgs a) {
  __shared__ DriveState rec;
  const int s = blockIdx.x, lane = threadIdx.x;
  // the state, read before anything of the scene is written (uniform: every lane holds it)
  const DriveState st = a.state[s];
  if (st.done != 0) {      // frozen
    if (lane == 0) a.done[s] = st.done;
    return;
  }
  const double* route = a.route + (size_t)s * a.G * 2;
  const double* cum = a.cum + (size_t)s * a.G;
  int len = a.len[s];
  len = len < 1 ? 1 : (len > a.G ? a.G : len);
  const double px = a.pose[(size_t)s * 3 + 0], py = a.pose[(size_t)s * 3 + 1];
  const double c2 = a.pose[(size_t)s * 3 + 2];
  const double compass = c2 != c2 ? 0.0 : c2;

  // ---- progress: the nearest point of the window ----
  int win_j = 0;
  double win_d = 0.0, win_t = 0.0, win_len = 0.0;
  if (len == 1) {
    win_d = norm2(px - route[0], py - route[1]);
  } else {
    const int cursor = st.cursor < 0 ? 0 : (st.cursor > len - 2 ? len - 2 : st.cursor);
    const int64_t far_end = (int64_t)cursor + a.window - 1;
    const int last = far_end < len - 2 ? (int)far_end : len - 2;      // >= cursor
    win_j = cursor;
    win_d = __builtin_inf();
    bool first = true;
    for (int base = cursor; base <= last; base += 64) {
      const int j = base + lane;
      double d = __builtin_inf(), t = 0.0, sl = 0.0;
      if (j <= last) {
        const double* p = route + (size_t)j * 2;      // j + 1 <= len - 1
        const double ax = p[0], ay = p[1];
        const double ux = p[2] - ax, uy = p[3] - ay;
        const double uxx = ux * ux, uyy = uy * uy;
        const double L2 = uxx + uyy;
        if (L2 > 0.0) {
          const double rx = px - ax, ry = py - ay;
          const double m0 = rx * ux, m1 = ry * uy;
          const double q = (m0 + m1) / L2;
          t = q > 0.0 ? (q < 1.0 ? q : 1.0) : 0.0;      // a NaN becomes 0
        }
        const double tx = t * ux, ty = t * uy;
        const double qx = ax + tx, qy = ay + ty;
        const double dd = norm2(px - qx, py - qy);
        d = dd != dd ? __builtin_inf() : dd;
        sl = sqrt(L2);
      }
      int idx = lane;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_xor(d, off, 64);
        const int oi = __shfl_xor(idx, off, 64);
        if (od < d || (od == d && oi < idx)) { d = od; idx = oi; }
      }
      if (first || d < win_d) {      // the first chunk's winner, then only a strictly nearer one
        win_d = d;
        win_j = base + idx;
        win_t = __shfl(t, idx, 64);
        win_len = __shfl(sl, idx, 64);
      }
      first = false;
    }
  }

  // ---- contact: lane j tests disc j and box j against the ego's discs ----
  const double fx = sin(compass), fy = -cos(compass);
  bool hit_disc = false, hit_box = false;
  if (lane < a.M) {
    const double* o = a.discs + ((size_t)s * a.M + lane) * 5;
    const double r = o[4];
    if (r > 0.0) {
      const double reach = r + a.r_ego;
      for (int k = 0; k < a.n_discs; ++k) {
        const double ox = a.offset[k] * fx, oy = a.offset[k] * fy;
        const double ex = px + ox, ey = py + oy;
        hit_disc = hit_disc || norm2(ex - o[0], ey - o[1]) < reach;
      }
    }
  }
  if (lane < a.N) {
    const double* o = a.boxes + ((size_t)s * a.N + lane) * 7;
    const double length = o[5], width = o[6];
    if (length > 0.0 && width > 0.0) {
      const double ux = cos(o[4]), uy = sin(o[4]);
      const double hl = length / 2.0, hw = width / 2.0;
      for (int k = 0; k < a.n_discs; ++k) {
        const double ox = a.offset[k] * fx, oy = a.offset[k] * fy;
        const double ex = (px + ox) - o[0], ey = (py + oy) - o[1];
        const double l0 = ex * ux, l1 = ey * uy;
        const double lx = l0 + l1;
        const double w0 = ex * uy, w1 = ey * ux;
        const double ly = -w0 + w1;
        const double qx = max0(fabs(lx) - hl), qy = max0(fabs(ly) - hw);
        hit_box = hit_box || norm2(qx, qy) < a.r_ego;
      }
    }
  }
  const unsigned long long disc_mask = __ballot(hit_disc), box_mask = __ballot(hit_box);
  const bool hit = (disc_mask | box_mask) != 0ull;
  const int slot = disc_mask != 0ull ? __ffsll((long long)disc_mask) - 1 : (box_mask != 0ull ? 64 + __ffsll((long long)box_mask) - 1 : 0);

  // ---- the record: sequential bookkeeping, lane 0 ----
  if (lane == 0) {
    DriveState n = st;
    const double length = cum[len - 1];
    n.cursor = win_j;
    const double along = win_t * win_len;
    n.progress = len == 1 ? 0.0 : cum[win_j] + along;
    n.progress_max = n.progress > st.progress_max ? n.progress : st.progress_max;
    n.xtrack = win_d;
    n.xtrack_max = win_d > st.xtrack_max ? win_d : st.xtrack_max;
    n.xtrack_sum = st.xtrack_sum + win_d;
    const double dsq = win_d * win_d;
    n.xtrack_sq = st.xtrack_sq + dsq;
    const double step = st.ticks > 0 ? norm2(px - st.px, py - st.py) : 0.0;
    n.distance = st.distance + step;
    n.px = px;
    n.py = py;
    // contact
    n.events = st.events + (hit && st.contact == 0 ? 1 : 0);
    n.contact_ticks = st.contact_ticks + (hit ? 1 : 0);
    n.contact = hit ? 1 : 0;
    n.ticks = st.ticks + 1;
    if (hit && st.first_tick == 0) {
      n.first_tick = n.ticks;
      n.first_slot = slot;
    }
    // route deviation
    bool off = win_d > a.offroad_max;
    if (win_d > a.offroad_min) {
      n.offroad = st.offroad + step;
      off = off || n.offroad / length > a.share;
    }
    // the stall clock
    const double v = (double)a.velocity[s];
    n.stall = v < a.speed_threshold ? st.stall + a.dt : 0.0;
    const bool blocked = n.stall > a.max_time;
    // comfort
    double acc = 0.0;
    if (st.have >= 1) {
      acc = (v - st.v_prev) / a.dt;
      const double mag = fabs(acc), sq = acc * acc;
      n.acc_max = mag > st.acc_max ? mag : st.acc_max;
      n.acc_sq = st.acc_sq + sq;
      n.a_prev = acc;
    }
    if (st.have >= 2) {
      const double jk = (acc - st.a_prev) / a.dt;
      const double mag = fabs(jk), sq = jk * jk;
      n.jerk_max = mag > st.jerk_max ? mag : st.jerk_max;
      n.jerk_sq = st.jerk_sq + sq;
    }
    const double lat = v * (double)a.yaw_rate[s];
    const double lmag = fabs(lat), lsq = lat * lat;
    n.lat_max = lmag > st.lat_max ? lmag : st.lat_max;
    n.lat_sq = st.lat_sq + lsq;
    n.v_prev = v;
    n.have = st.have >= 2 ? 2 : st.have + 1;
    // done: the first condition that holds; flags: every one that holds
    const bool cond[5] = {n.progress_max >= length - a.completion_tol, hit && a.stop_on_collision != 0, off, blocked,
                          a.max_ticks > 0 && n.ticks >= a.max_ticks};
    int done = 0, flags = 0;
#pragma unroll
    for (int i = 4; i >= 0; --i)
      if (cond[i]) {
        done = i + 1;
        flags |= 1 << i;
      }
    n.done = done;
    n.flags = flags;
    rec = n;
    a.done[s] = done;
  }
  __syncthreads();
  if (lane < kDriveWords) reinterpret_cast<uint32_t*>(a.state + s)[lane] = reinterpret_cast<const uint32_t*>(&rec)[lane];
}

__global__ void __launch_bounds__(256) drive_reset_kernel(uint32_t* state, const uint8_t* mask, int32_t* done, int scenes) {
  const int i = blockIdx.x * 256 + threadIdx.x;      // scenes * 48 < 2^22
  if (i >= scenes * kDriveWords) return;
  const int s = i / kDriveWords;
  if (mask != nullptr && mask[s] == 0) return;
  state[i] = 0u;
  if (done != nullptr && i % kDriveWords == 0) done[s] = 0;
}

bool finite_pos(double v) { return v > 0.0 && v < __builtin_inf(); }
bool finite_nonneg(double v) { return v >= 0.0 && v < __builtin_inf(); }

}  // namespace

size_t drive_state_bytes(int scenes) { return scenes >= 1 && scenes <= kDriveMaxScenes ? (size_t)scenes * sizeof(DriveState) : 0; }

int drive_reset(void* state, int scenes, const uint8_t* mask, int32_t* done, hipStream_t s) {
  ADX_REQUIRE(scenes >= 1 && scenes <= kDriveMaxScenes, "drive reset: %d scenes, supported 1..%d", scenes, kDriveMaxScenes);
  ADX_REQUIRE(state != nullptr, "drive reset: null state");
  const size_t nb = drive_state_bytes(scenes), db = (size_t)scenes * sizeof(int32_t);
  ADX_REQUIRE(mask == nullptr || !byte_ranges_overlap(state, nb, mask, (size_t)scenes), "drive reset: the mask overlaps the state");
  ADX_REQUIRE(done == nullptr || !byte_ranges_overlap(state, nb, done, db), "drive reset: done overlaps the state");
  ADX_REQUIRE(done == nullptr || mask == nullptr || !byte_ranges_overlap(done, db, mask, (size_t)scenes),
              "drive reset: the mask overlaps done");
  drive_reset_kernel<<<dim3(ceil_div(scenes * kDriveWords, 256)), dim3(256), 0, s>>>(static_cast<uint32_t*>(state), mask, done, scenes);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

int drive_step(const adx_drive_cfg* c, const double* pose, const float* velocity, const float* yaw_rate, const double* route,
               const int32_t* len, const double* cum, const double* discs, const double* boxes, void* state, int32_t* done,
               hipStream_t s) {
  ADX_REQUIRE(c != nullptr, "drive step: null configuration");
  const int S = c->scenes, G = c->max_points, M = c->n_world_discs, N = c->n_boxes;
  ADX_REQUIRE(S >= 1 && S <= kDriveMaxScenes, "drive step: %d scenes, supported 1..%d", S, kDriveMaxScenes);
  ADX_REQUIRE(G >= 1 && G <= kDriveMaxPoints, "drive step: %d route points, supported 1..%d", G, kDriveMaxPoints);
  ADX_REQUIRE(c->window >= 1 && c->window <= kDriveMaxPoints, "drive step: a window of %d segments, supported 1..%d", c->window,
              kDriveMaxPoints);
  ADX_REQUIRE(M >= 0 && M <= kDriveMaxSlots, "drive step: %d world discs, supported 0..%d", M, kDriveMaxSlots);
  ADX_REQUIRE(N >= 0 && N <= kDriveMaxSlots, "drive step: %d boxes, supported 0..%d", N, kDriveMaxSlots);
  ADX_REQUIRE(c->n_discs >= 1 && c->n_discs <= 4, "drive step: an ego of %d discs, supported 1..4", c->n_discs);
  ADX_REQUIRE(c->max_ticks >= 0, "drive step: max_ticks %d must be >= 0 (0: no timeout)", c->max_ticks);
  ADX_REQUIRE(finite_pos(c->dt), "drive step: dt %g must be finite and > 0", c->dt);
  const double nonneg[7] = {c->r_ego, c->offroad_min, c->offroad_max, c->max_route_percentage, c->speed_threshold, c->max_time,
                            c->completion_tol};
  const char* const nn_names[7] = {"r_ego", "offroad_min", "offroad_max", "max_route_percentage", "speed_threshold", "max_time",
                                   "completion_tol"};
  for (int i = 0; i < 7; ++i) ADX_REQUIRE(finite_nonneg(nonneg[i]), "drive step: %s %g must be finite and >= 0", nn_names[i], nonneg[i]);
  for (int k = 0; k < c->n_discs; ++k)
    ADX_REQUIRE(c->offset[k] > -__builtin_inf() && c->offset[k] < __builtin_inf(), "drive step: offset[%d] %g must be finite", k,
                c->offset[k]);
  ADX_REQUIRE((discs != nullptr) == (M > 0), "drive step: discs must be given exactly when n_world_discs > 0 (%d)", M);
  ADX_REQUIRE((boxes != nullptr) == (N > 0), "drive step: boxes must be given exactly when n_boxes > 0 (%d)", N);
  const ByteSpan ins[8] = {{pose, (size_t)S * 3 * sizeof(double)},      {velocity, (size_t)S * sizeof(float)},
                           {yaw_rate, (size_t)S * sizeof(float)},       {route, (size_t)S * G * 2 * sizeof(double)},
                           {len, (size_t)S * sizeof(int32_t)},          {cum, (size_t)S * G * sizeof(double)},
                           {discs, (size_t)S * M * 5 * sizeof(double)}, {boxes, (size_t)S * N * 7 * sizeof(double)}};
  const char* const in_names[8] = {"pose", "velocity", "yaw_rate", "route", "len", "cum", "discs", "boxes"};
  for (int j = 0; j < 6; ++j) ADX_REQUIRE(ins[j].p != nullptr, "drive step: null %s", in_names[j]);
  ADX_REQUIRE(state != nullptr, "drive step: null state");
  ADX_REQUIRE(done != nullptr, "drive step: null done");
  const size_t nb = drive_state_bytes(S), db = (size_t)S * sizeof(int32_t);
  for (int j = 0; j < 8; ++j) {
    if (ins[j].p == nullptr) continue;
    ADX_REQUIRE(!byte_ranges_overlap(state, nb, ins[j].p, ins[j].n), "drive step: the state aliases %s", in_names[j]);
    ADX_REQUIRE(!byte_ranges_overlap(done, db, ins[j].p, ins[j].n), "drive step: done aliases %s", in_names[j]);
  }
  ADX_REQUIRE(!byte_ranges_overlap(state, nb, done, db), "drive step: done aliases the state");
  DriveArgs a = {};
  a.pose = pose; a.velocity = velocity; a.yaw_rate = yaw_rate; a.route = route; a.len = len; a.cum = cum; a.discs = discs; a.boxes = boxes;
  a.state = static_cast<DriveState*>(state);
  a.done = done;
  a.G = G; a.window = c->window; a.M = M; a.N = N; a.n_discs = c->n_discs; a.stop_on_collision = c->stop_on_collision;
  a.max_ticks = c->max_ticks;
  a.dt = c->dt; a.r_ego = c->r_ego;
  for (int k = 0; k < 4; ++k) a.offset[k] = k < c->n_discs ? c->offset[k] : 0.0;
  a.offroad_min = c->offroad_min; a.offroad_max = c->offroad_max; a.share = c->max_route_percentage;
  a.speed_threshold = c->speed_threshold; a.max_time = c->max_time; a.completion_tol = c->completion_tol;
  drive_step_kernel<<<dim3(S), dim3(64), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

}  // namespace adx
