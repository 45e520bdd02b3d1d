// Who else is on the road (include/adx.h: "traffic v1"): car-following agents on caller-laid paths -- the Intelligent Driver Model
// behind the nearest of another agent, the ego and a red or yellow stop line -- advanced by one tick per launch with their state
// in device memory, and written out as the boxes `World`, ego frame v1 and drive metrics v1 take.
//
// fp64, no contraction, no library call (only + - * / and sqrt), latency-bound like drive.hip and signals.hip, and laid out like
// them:
//   traffic_step_kernel   one workgroup of one wave per scene, lane i owns agent i.  The scene's paths (points, arc lengths,
//                         headings: at most 16 KB) are staged into LDS once.  The ego is projected onto one path at a time, lanes
//                         over segments, with drive.hip's xor butterfly over (d, j).  The leader search is a uniform loop over k
//                         with a cross-lane broadcast of lane k's (path, s, v, rear); the stops are read once, lane t stop t
//                         and its phase, and are then a short uniform loop over LDS.  The record's counters are population
//                         counts of ballots; lane 0 forms the record in LDS, then lanes 0 .. 31 store one 32-bit word of it each,
//                         and every lane stores its agent and its box word by word (narrow stores, for vehicle.hip's reason).
//   traffic_reset_kernel  the same staging; the masked scenes' agents go to their starts and their boxes are written.
// No atomics, no traffic between workgroups: the same inputs and state give the same bits on every launch.
#include "sched.h"

#pragma clang fp contract(off)

namespace adx {

namespace {

constexpr int kTrMaxScenes = 65535, kTrMaxAgents = 64, kTrMaxPaths = 8, kTrMaxPoints = 64, kTrMaxStops = 16, kTrMaxSignals = 64;
constexpr int kTrAgentWidth = 9, kTrBoxWidth = 7, kTrHead = 32;      // 32 words of record in front of the agents
constexpr int kYellow = 2, kRed = 3, kEgo = 64;
constexpr int kStageRounds = kTrMaxPaths * kTrMaxPoints / 64;      // rounds of 64 lanes over a table of Q * G values

// words of a scene's state: 0 ticks, 1 have, 2 arrived, 3 ego_yields, 4 ego_hard, 5 overlaps, 6..7 min_ego_gap, 8..23 se_prev[8],
// 24..31 on_prev[8], then s[N] fp64, v[N] fp64, alive[N] int32 and a zero word when N is odd
__host__ __device__ inline int traffic_words(int N) { return kTrHead + 5 * N + (N & 1); }

struct TrArgs {
  const double* paths;        // [S][Q][G][2]
  const int32_t* plen;        // [S][Q]
  const double* cum;          // [S][Q][G]
  const double* heading;      // [S][Q][G]
  const double* agents;       // [S][N][9]
  const double* stops;        // [S][T][3] or null
  const int32_t* phase;       // [S][n_signals] or null
  const double* pose;         // [S][3]
  const int32_t* hold;        // [S] or null
  const uint8_t* mask;        // [S] or null (reset)
  uint32_t* state;            // [S][words]
  double* boxes;              // [S][N][7]
  int32_t* leader;            // [S][N] (reset: or null)
  int N, Q, G, T, n_signals;
  double dt, lane_half_width, ego_length, jam, gap_min, brake_max;
};

// one 32-bit word per lane and store instruction: volatile keeps the compiler from merging neighbours into a wide store
__device__ __forceinline__ void put32(void* base, int word, uint32_t v) { reinterpret_cast<volatile uint32_t*>(base)[word] = v; }

__device__ __forceinline__ void put64(void* base, int word, double v) {
  const unsigned long long bits = __builtin_bit_cast(unsigned long long, v);
  put32(base, word, (uint32_t)bits);
  put32(base, word + 1, (uint32_t)(bits >> 32));
}

__device__ __forceinline__ double get64(const uint32_t* base, int word) {
  return __builtin_bit_cast(double, (unsigned long long)base[word] | ((unsigned long long)base[word + 1] << 32));
}

// lane k's value for every lane, k the same in all of them
__device__ __forceinline__ double lane_value(double v, int k) {
  const unsigned long long bits = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(uint32_t)bits, k);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(uint32_t)(bits >> 32), k);
  return __builtin_bit_cast(double, (unsigned long long)lo | ((unsigned long long)hi << 32));
}

struct TrPaths {      // a scene's paths in LDS
  double p[kTrMaxPaths * kTrMaxPoints * 2], cum[kTrMaxPaths * kTrMaxPoints], heading[kTrMaxPaths * kTrMaxPoints];
  int len[kTrMaxPaths];
};

__device__ __forceinline__ void stage_paths(const TrArgs& a, int s, int lane, TrPaths& sp) {
  const int QG = a.Q * a.G;      // <= 512
  const double* p = a.paths + (size_t)s * QG * 2;
  const double* c = a.cum + (size_t)s * QG;
  const double* h = a.heading + (size_t)s * QG;
  // every load of a table is issued before its first store to LDS: the launch is made of latencies, and 32 loads one after the
  // other would be most of it
  double rp[2 * kStageRounds], rc[kStageRounds], rh[kStageRounds];
#pragma unroll
  for (int k = 0; k < 2 * kStageRounds; ++k) rp[k] = lane + 64 * k < QG * 2 ? p[lane + 64 * k] : 0.0;
#pragma unroll
  for (int k = 0; k < kStageRounds; ++k) {
    rc[k] = lane + 64 * k < QG ? c[lane + 64 * k] : 0.0;
    rh[k] = lane + 64 * k < QG ? h[lane + 64 * k] : 0.0;
  }
#pragma unroll
  for (int k = 0; k < 2 * kStageRounds; ++k)
    if (lane + 64 * k < QG * 2) sp.p[lane + 64 * k] = rp[k];
#pragma unroll
  for (int k = 0; k < kStageRounds; ++k)
    if (lane + 64 * k < QG) {
      sp.cum[lane + 64 * k] = rc[k];
      sp.heading[lane + 64 * k] = rh[k];
    }
  if (lane < a.Q) {
    const int l = a.plen[(size_t)s * a.Q + lane];
    sp.len[lane] = l < 0 ? 0 : (l > a.G ? a.G : l);
  }
  __syncthreads();
}

struct TrSlot {      // "agents" of traffic v1: one row, and whether it is a slot at all
  bool valid;
  int path;
  double start_s, start_v, desired, length, width, headway, accel, brake;
};

__device__ __forceinline__ TrSlot read_slot(const TrArgs& a, int s, int lane, const TrPaths& sp) {
  TrSlot o = {};
  if (lane >= a.N) return o;
  const double* g = a.agents + ((size_t)s * a.N + lane) * kTrAgentWidth;
  const double pf = g[0];
  o.start_s = g[1]; o.start_v = g[2]; o.desired = g[3]; o.length = g[4]; o.width = g[5]; o.headway = g[6]; o.accel = g[7]; o.brake = g[8];
  if (!(pf >= 0.0 && pf <= (double)(a.Q - 1))) return o;
  const int q = (int)pf;      // 0 .. Q-1
  if ((double)q != pf || sp.len[q] < 2) return o;
  o.path = q;
  o.valid = o.length > 0.0 && o.width > 0.0 && o.desired > 0.0 && o.accel > 0.0 && o.brake > 0.0 && o.headway >= 0.0 &&
            o.start_s >= 0.0 && o.start_v >= 0.0 && o.start_s < sp.cum[q * a.G + sp.len[q] - 1];
  return o;
}

// "boxes" of traffic v1: lane's box from (s, v) on its path, or zeros
__device__ __forceinline__ void put_box(const TrArgs& a, int s, int lane, const TrPaths& sp, const TrSlot& sl, bool live, double as,
                                        double av) {
  if (lane >= a.N) return;
  double* o = a.boxes + ((size_t)s * a.N + lane) * kTrBoxWidth;
  double cx = 0.0, cy = 0.0, vx = 0.0, vy = 0.0, yaw = 0.0, length = 0.0, width = 0.0;
  if (live) {
    const int base = sl.path * a.G, last = sp.len[sl.path] - 2;      // >= 0
    int j = 0;
    for (int i = 1; i <= last; ++i)
      if (sp.cum[base + i] <= as) j = i;
    const double ax = sp.p[(base + j) * 2], ay = sp.p[(base + j) * 2 + 1];
    const double dx = sp.p[(base + j + 1) * 2] - ax, dy = sp.p[(base + j + 1) * 2 + 1] - ay;      // j + 1 <= len - 1
    const double dxx = dx * dx, dyy = dy * dy;
    const double L = sqrt(dxx + dyy);
    double ux = 0.0, uy = 0.0;
    if (L > 0.0) {
      ux = dx / L;
      uy = dy / L;
    }
    const double along = as - sp.cum[base + j];
    const double ox = along * ux, oy = along * uy;
    cx = ax + ox;
    cy = ay + oy;
    vx = av * ux;
    vy = av * uy;
    yaw = sp.heading[base + j];
    length = sl.length;
    width = sl.width;
  }
  put64(o, 0, cx);
  put64(o, 2, cy);
  put64(o, 4, vx);
  put64(o, 6, vy);
  put64(o, 8, yaw);
  put64(o, 10, length);
  put64(o, 12, width);
}

__global__ void __launch_bounds__(64) traffic_step_kernel(const TrArgs a) {
  __shared__ TrPaths sp;
  __shared__ double e_se[kTrMaxPaths], e_ue[kTrMaxPaths];
  __shared__ int e_on[kTrMaxPaths];
  __shared__ double stop_path[kTrMaxStops], stop_s[kTrMaxStops];
  __shared__ int stop_phase[kTrMaxStops];
  __shared__ uint32_t rec[kTrHead];
  const int s = blockIdx.x, lane = threadIdx.x, N = a.N;
  uint32_t* st = a.state + (size_t)s * traffic_words(N);
  // the state, read before anything of the scene is written: the record by every lane (uniform), agent `lane` by its lane
  const int have = (int)st[1];      // have == 0: a fresh state is the state a reset leaves, whatever its other words hold
  const int ticks0 = have != 0 ? (int)st[0] : 0, arrived0 = have != 0 ? (int)st[2] : 0, yields0 = have != 0 ? (int)st[3] : 0;
  const int hard0 = have != 0 ? (int)st[4] : 0, overlaps0 = have != 0 ? (int)st[5] : 0;
  const double min_gap0 = have != 0 ? get64(st, 6) : __builtin_inf();
  double se_prev = 0.0;
  int on_prev = 0;
  if (lane < kTrMaxPaths) {
    se_prev = get64(st, 8 + 2 * lane);
    on_prev = have != 0 ? (int)st[24 + lane] : 0;
  }
  double as = 0.0, av = 0.0;
  int alive = 0;
  if (lane < N) {
    as = get64(st, kTrHead + 2 * lane);
    av = get64(st, kTrHead + 2 * N + 2 * lane);
    alive = (int)st[kTrHead + 4 * N + lane];
  }
  const bool held = a.hold != nullptr && a.hold[s] != 0;
  stage_paths(a, s, lane, sp);
  const TrSlot sl = read_slot(a, s, lane, sp);
  if (have == 0) {
    as = sl.valid ? sl.start_s : 0.0;
    av = sl.valid ? sl.start_v : 0.0;
    alive = sl.valid ? 1 : 0;
  }
  const bool live = alive != 0 && sl.valid;
  if (held) {      // frozen: the boxes are written again from the state as it stands
    put_box(a, s, lane, sp, sl, live, as, av);
    return;
  }

  // ---- the ego on every path: lanes over segments ----
  const double px = a.pose[(size_t)s * 3 + 0], py = a.pose[(size_t)s * 3 + 1];
  for (int q = 0; q < a.Q; ++q) {
    const int len = sp.len[q], base = q * a.G;
    double se = 0.0, ue = 0.0;
    int on = 0;
    if (len >= 2) {      // uniform
      double d = __builtin_inf(), t = 0.0, sg = 0.0;
      if (lane <= len - 2) {
        const double ax = sp.p[(base + lane) * 2], ay = sp.p[(base + lane) * 2 + 1];
        const double ux = sp.p[(base + lane + 1) * 2] - ax, uy = sp.p[(base + lane + 1) * 2 + 1] - ay;
        const double uxx = ux * ux, uyy = uy * uy;
        const double L2 = uxx + uyy;
        if (L2 > 0.0) {
          const double rx = px - ax, ry = py - ay;
          const double m0 = rx * ux, m1 = ry * uy;
          const double f = (m0 + m1) / L2;
          t = f > 0.0 ? (f < 1.0 ? f : 1.0) : 0.0;      // a NaN becomes 0
        }
        const double tx = t * ux, ty = t * uy;
        const double qx = ax + tx, qy = ay + ty;
        const double ex = px - qx, ey = py - qy;
        const double exx = ex * ex, eyy = ey * ey;
        const double dd = sqrt(exx + eyy);
        d = dd != dd ? __builtin_inf() : dd;
        sg = sqrt(L2);
      }
      int idx = lane;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_xor(d, off, 64);
        const int oi = __shfl_xor(idx, off, 64);
        if (od < d || (od == d && oi < idx)) { d = od; idx = oi; }
      }
      const double wt = __shfl(t, idx, 64), wl = __shfl(sg, idx, 64);
      const double along = wt * wl;
      se = sp.cum[base + idx] + along;      // idx <= len - 2: the lanes past it hold +inf and a higher index
      on = d <= a.lane_half_width ? 1 : 0;
      const int was = __shfl(on_prev, q, 64);
      const double prev = __shfl(se_prev, q, 64);
      if (on != 0 && was != 0) {
        const double r = (se - prev) / a.dt;
        ue = r > 0.0 ? r : 0.0;
      }
    }
    if (lane == 0) {
      e_se[q] = se;
      e_ue[q] = ue;
      e_on[q] = on;
    }
  }
  // the stops and the phases they read, lane t stop t: two loads in a row for the scene instead of two per stop and agent
  if (lane < a.T) {
    const double* g = a.stops + ((size_t)s * a.T + lane) * 3;
    const double sf = g[2];
    int ph = 0;
    if (sf >= 0.0 && sf <= (double)(a.n_signals - 1)) {
      const int slot = (int)sf;      // 0 .. n_signals-1
      if ((double)slot == sf) ph = a.phase[(size_t)s * a.n_signals + slot];
    }
    stop_path[lane] = g[0];
    stop_s[lane] = g[1];
    stop_phase[lane] = ph;
  }
  __syncthreads();

  // ---- the leader of agent `lane` ----
  const double half = sl.length / 2.0;
  const double front = as + half;
  const double rear = as - half;
  const int my_path = live ? sl.path : -1;
  double best_r = __builtin_inf(), best_u = 0.0;
  int lead = -1;
  for (int k = 0; k < N; ++k) {
    const int kp = __builtin_amdgcn_readlane(my_path, k);      // k is uniform: a register read, not a trip through LDS
    const double ks = lane_value(as, k), kv = lane_value(av, k), kr = lane_value(rear, k);
    if (live && kp == my_path && k != lane && (ks > as || (ks == as && k < lane)) && kr < best_r) {
      best_r = kr;
      best_u = kv;
      lead = k;
    }
  }
  if (live) {
    if (e_on[sl.path] != 0 && e_se[sl.path] > as) {
      const double r = e_se[sl.path] - a.ego_length / 2.0;
      if (r < best_r) {
        best_r = r;
        best_u = e_ue[sl.path];
        lead = kEgo;
      }
    }
    const double b2 = 2.0 * sl.brake, vv = av * av;
    for (int t = 0; t < a.T; ++t) {
      const double ss = stop_s[t];
      const int ph = stop_phase[t];      // 0 where the slot is out of range: inert
      if (!(stop_path[t] == (double)sl.path && front <= ss)) continue;
      bool binds = ph == kRed;
      if (ph == kYellow) {
        const double room = (ss - front) * b2;
        binds = room >= vv;
      }
      if (binds && ss < best_r) {
        best_r = ss;
        best_u = 0.0;
        lead = kEgo + 1 + t;
      }
    }
  }

  // ---- the law ----
  double ns = as, nv = av, gap = __builtin_inf();
  bool hard = false, arrive = false;
  if (live) {
    const double f = av / sl.desired;
    const double f2 = f * f;
    const double f4 = f2 * f2;
    const double free_ = 1.0 - f4;
    double inter = 0.0;
    if (lead >= 0) {
      gap = best_r - front;
      const double ab = sl.accel * sl.brake;
      const double den = 2.0 * sqrt(ab);
      const double t0 = av * sl.headway;
      const double dv = av - best_u;
      const double t1 = av * dv;
      const double t2 = t1 / den;
      const double dyn = t0 + t2;
      const double star = a.jam + (dyn > 0.0 ? dyn : 0.0);
      const double g = gap > a.gap_min ? gap : a.gap_min;
      const double ratio = star / g;
      inter = ratio * ratio;
    }
    double acc = sl.accel * (free_ - inter);
    if (acc < -a.brake_max) {
      acc = -a.brake_max;
      hard = true;
    }
    if (acc > sl.accel) acc = sl.accel;
    const double dvv = acc * a.dt;
    const double v1 = av + dvv;
    nv = v1 > 0.0 ? v1 : 0.0;
    const double ds = nv * a.dt;
    ns = as + ds;
    arrive = ns >= sp.cum[sl.path * a.G + sp.len[sl.path] - 1];
  }
  const bool by_ego = live && lead == kEgo;
  const unsigned long long yield_mask = __ballot(by_ego), hard_mask = __ballot(by_ego && hard);
  const unsigned long long over_mask = __ballot(live && lead >= 0 && lead < kEgo && gap < 0.0), arrive_mask = __ballot(arrive);
  double mg = by_ego && gap == gap ? gap : __builtin_inf();
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double og = __shfl_xor(mg, off, 64);
    if (og < mg) mg = og;
  }

  // ---- the record: lane 0 ----
  if (lane == 0) {
    rec[0] = (uint32_t)(ticks0 + 1);
    rec[1] = 1u;
    rec[2] = (uint32_t)(arrived0 + __popcll(arrive_mask));
    rec[3] = (uint32_t)(yields0 + __popcll(yield_mask));
    rec[4] = (uint32_t)(hard0 + __popcll(hard_mask));
    rec[5] = (uint32_t)(overlaps0 + __popcll(over_mask));
    const unsigned long long mb = __builtin_bit_cast(unsigned long long, mg < min_gap0 ? mg : min_gap0);
    rec[6] = (uint32_t)mb;
    rec[7] = (uint32_t)(mb >> 32);
    for (int q = 0; q < kTrMaxPaths; ++q) {
      const bool in = q < a.Q;
      const unsigned long long sb = __builtin_bit_cast(unsigned long long, in ? e_se[q] : 0.0);
      rec[8 + 2 * q] = (uint32_t)sb;
      rec[9 + 2 * q] = (uint32_t)(sb >> 32);
      rec[24 + q] = in ? (uint32_t)e_on[q] : 0u;
    }
  }
  __syncthreads();
  if (lane < kTrHead) put32(st, lane, rec[lane]);
  const bool stays = live && !arrive;
  if (lane < N) {
    put64(st, kTrHead + 2 * lane, ns);
    put64(st, kTrHead + 2 * N + 2 * lane, nv);
    put32(st, kTrHead + 4 * N + lane, stays ? 1u : 0u);
    a.leader[(size_t)s * N + lane] = live ? lead : -1;
  }
  if (lane == 0 && (N & 1) != 0) put32(st, kTrHead + 5 * N, 0u);
  put_box(a, s, lane, sp, sl, stays, ns, nv);
}

__global__ void __launch_bounds__(64) traffic_reset_kernel(const TrArgs a) {
  __shared__ TrPaths sp;
  const int s = blockIdx.x, lane = threadIdx.x, N = a.N;
  if (a.mask != nullptr && a.mask[s] == 0) return;      // uniform
  stage_paths(a, s, lane, sp);
  const TrSlot sl = read_slot(a, s, lane, sp);
  uint32_t* st = a.state + (size_t)s * traffic_words(N);
  if (lane < kTrHead) {
    const unsigned long long inf = __builtin_bit_cast(unsigned long long, __builtin_inf());
    put32(st, lane, lane == 1 ? 1u : (lane == 6 ? (uint32_t)inf : (lane == 7 ? (uint32_t)(inf >> 32) : 0u)));
  }
  if (lane < N) {
    put64(st, kTrHead + 2 * lane, sl.valid ? sl.start_s : 0.0);
    put64(st, kTrHead + 2 * N + 2 * lane, sl.valid ? sl.start_v : 0.0);
    put32(st, kTrHead + 4 * N + lane, sl.valid ? 1u : 0u);
    if (a.leader != nullptr) a.leader[(size_t)s * N + lane] = -1;
  }
  if (lane == 0 && (N & 1) != 0) put32(st, kTrHead + 5 * N, 0u);
  put_box(a, s, lane, sp, sl, sl.valid, sl.start_s, sl.start_v);
}

bool finite_pos(double v) { return v > 0.0 && v < __builtin_inf(); }

// what step and reset share: the limits, the tables and the outputs
int traffic_check(const char* who, const adx_traffic_cfg* c, const double* paths, const int32_t* plen, const double* cum,
                  const double* heading, const double* agents, const ByteSpan* more, const char* const* more_names, int n_more,
                  void* state, double* boxes, int32_t* leader, bool leader_needed) {
  ADX_REQUIRE(c != nullptr, "%s: null configuration", who);
  const int S = c->scenes, N = c->n_agents, Q = c->n_paths, G = c->n_points, T = c->n_stops;
  ADX_REQUIRE(S >= 1 && S <= kTrMaxScenes, "%s: %d scenes, supported 1..%d", who, S, kTrMaxScenes);
  ADX_REQUIRE(N >= 1 && N <= kTrMaxAgents, "%s: %d agents, supported 1..%d", who, N, kTrMaxAgents);
  ADX_REQUIRE(Q >= 1 && Q <= kTrMaxPaths, "%s: %d paths, supported 1..%d", who, Q, kTrMaxPaths);
  ADX_REQUIRE(G >= 2 && G <= kTrMaxPoints, "%s: %d path points, supported 2..%d", who, G, kTrMaxPoints);
  ADX_REQUIRE(T >= 0 && T <= kTrMaxStops, "%s: %d stops, supported 0..%d", who, T, kTrMaxStops);
  ADX_REQUIRE(c->n_signals >= (T > 0 ? 1 : 0) && c->n_signals <= kTrMaxSignals, "%s: %d signals, supported %d..%d with %d stops", who,
              c->n_signals, T > 0 ? 1 : 0, kTrMaxSignals, T);
  const double pos[6] = {c->dt, c->lane_half_width, c->ego_length, c->jam, c->gap_min, c->brake_max};
  const char* const pos_names[6] = {"dt", "lane_half_width", "ego_length", "jam", "gap_min", "brake_max"};
  for (int i = 0; i < 6; ++i) ADX_REQUIRE(finite_pos(pos[i]), "%s: %s %g must be finite and > 0", who, pos_names[i], pos[i]);
  ByteSpan ins[12] = {{paths, (size_t)S * Q * G * 2 * sizeof(double)},
                      {plen, (size_t)S * Q * sizeof(int32_t)},
                      {cum, (size_t)S * Q * G * sizeof(double)},
                      {heading, (size_t)S * Q * G * sizeof(double)},
                      {agents, (size_t)S * N * kTrAgentWidth * sizeof(double)}};
  const char* in_names[12] = {"paths", "plen", "cum", "heading", "agents"};
  for (int j = 0; j < 5; ++j) ADX_REQUIRE(ins[j].p != nullptr, "%s: null %s", who, in_names[j]);
  for (int j = 0; j < n_more; ++j) {
    ins[5 + j] = more[j];
    in_names[5 + j] = more_names[j];
  }
  const ByteSpan outs[3] = {{state, traffic_state_bytes(S, N)},
                            {boxes, (size_t)S * N * kTrBoxWidth * sizeof(double)},
                            {leader, (size_t)S * N * sizeof(int32_t)}};
  const char* const names[3] = {"the state", "boxes", "leader"};
  ADX_REQUIRE(state != nullptr, "%s: null state", who);
  ADX_REQUIRE(boxes != nullptr, "%s: null boxes", who);
  ADX_REQUIRE(leader != nullptr || !leader_needed, "%s: null leader", who);
  for (int i = 0; i < 3; ++i) {
    if (outs[i].p == nullptr) continue;
    for (int j = 0; j < 5 + n_more; ++j)
      ADX_REQUIRE(ins[j].p == nullptr || !byte_ranges_overlap(outs[i].p, outs[i].n, ins[j].p, ins[j].n), "%s: %s aliases %s", who, names[i],
                  in_names[j]);
    for (int j = 0; j < i; ++j)
      ADX_REQUIRE(!byte_ranges_overlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n), "%s: %s and %s alias each other", who, names[j],
                  names[i]);
  }
  return ADX_OK;
}

TrArgs traffic_args(const adx_traffic_cfg* c, const double* paths, const int32_t* plen, const double* cum, const double* heading,
                    const double* agents, void* state, double* boxes, int32_t* leader) {
  TrArgs a = {};
  a.paths = paths; a.plen = plen; a.cum = cum; a.heading = heading; a.agents = agents;
  a.state = static_cast<uint32_t*>(state);
  a.boxes = boxes; a.leader = leader;
  a.N = c->n_agents; a.Q = c->n_paths; a.G = c->n_points; a.T = c->n_stops; a.n_signals = c->n_signals;
  a.dt = c->dt; a.lane_half_width = c->lane_half_width; a.ego_length = c->ego_length; a.jam = c->jam; a.gap_min = c->gap_min;
  a.brake_max = c->brake_max;
  return a;
}

}  // namespace

size_t traffic_state_bytes(int scenes, int n_agents) {
  return scenes >= 1 && scenes <= kTrMaxScenes && n_agents >= 1 && n_agents <= kTrMaxAgents ? (size_t)scenes * traffic_words(n_agents) * 4 : 0;
}

int traffic_reset(const adx_traffic_cfg* c, const double* paths, const int32_t* plen, const double* cum, const double* heading,
                  const double* agents, const uint8_t* mask, void* state, double* boxes, int32_t* leader, hipStream_t s) {
  const ByteSpan more[1] = {{mask, c == nullptr ? 0 : (size_t)(c->scenes > 0 ? c->scenes : 0)}};
  const char* const more_names[1] = {"the mask"};
  const int rc = traffic_check("traffic reset", c, paths, plen, cum, heading, agents, more, more_names, 1, state, boxes, leader, false);
  if (rc != ADX_OK) return rc;
  TrArgs a = traffic_args(c, paths, plen, cum, heading, agents, state, boxes, leader);
  a.mask = mask;
  traffic_reset_kernel<<<dim3(c->scenes), dim3(64), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

int traffic_step(const adx_traffic_cfg* c, const double* paths, const int32_t* plen, const double* cum, const double* heading,
                 const double* agents, const double* stops, const int32_t* phase, const double* pose, const float* velocity,
                 const int32_t* hold, void* state, double* boxes, int32_t* leader, hipStream_t s) {
  const size_t S = c == nullptr || c->scenes < 0 ? 0 : (size_t)c->scenes, T = c == nullptr || c->n_stops < 0 ? 0 : (size_t)c->n_stops;
  const size_t n_sig = c == nullptr || c->n_signals < 0 ? 0 : (size_t)c->n_signals;
  const ByteSpan more[5] = {{stops, S * T * 3 * sizeof(double)},
                            {phase, S * n_sig * sizeof(int32_t)},
                            {pose, S * 3 * sizeof(double)},
                            {velocity, S * sizeof(float)},
                            {hold, S * sizeof(int32_t)}};
  const char* const more_names[5] = {"stops", "phase", "pose", "velocity", "hold"};
  const int rc = traffic_check("traffic step", c, paths, plen, cum, heading, agents, more, more_names, 5, state, boxes, leader, true);
  if (rc != ADX_OK) return rc;
  ADX_REQUIRE((stops != nullptr) == (c->n_stops > 0), "traffic step: stops must be given exactly when n_stops > 0 (%d)", c->n_stops);
  ADX_REQUIRE((phase != nullptr) == (c->n_stops > 0), "traffic step: phase must be given exactly when n_stops > 0 (%d)", c->n_stops);
  ADX_REQUIRE(pose != nullptr, "traffic step: null pose");
  ADX_REQUIRE(velocity != nullptr, "traffic step: null velocity");
  TrArgs a = traffic_args(c, paths, plen, cum, heading, agents, state, boxes, leader);
  a.stops = stops; a.phase = phase; a.pose = pose; a.hold = hold;      // v1 carries `velocity` and does not read it
  traffic_step_kernel<<<dim3(c->scenes), dim3(64), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

}  // namespace adx
