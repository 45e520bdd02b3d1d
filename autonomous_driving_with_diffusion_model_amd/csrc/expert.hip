// A privileged driver (include/adx.h: "expert v1"): for every scene the route window, the speed and the world in the tick's ego
// frame go in; the plan control v1 takes, the leader it queues behind and an 8-word record of why come out.  Stateless.
//
// fp64, no contraction, no library call (only + - * / and sqrt), latency-bound like traffic.hip and drive.hip, and laid out like
// them:
//   expert_plan_kernel   one workgroup of one wave per scene.  The window is staged into LDS once: lane i point i, then lane j
//                        segment j (its vector, squared length, length and tangent), then lane 0 the sequential arc lengths --
//                        2.4 KB (nine tables of 32 doubles and one of 32 ints).  Every lane projects the ego (a uniform loop over at most 31 segments; the result is the same
//                        in all of them, so nothing is broadcast).  Lane i then owns box i, disc i, plane i and curve vertex i,
//                        each a uniform loop over the segments in LDS; one xor butterfly takes the minimum over (r, leader code)
//                        -- the codes are in the contract's candidate order, so the earlier candidate wins a tie -- and one the
//                        smallest curve limit.  The H-step roll-out runs REDUNDANTLY in every lane: a wave takes one lane's
//                        dependent chain in the time of 64, and lane k keeps a_k in a register as the loop passes k, so the
//                        rows need no LDS round trip and no barrier; lane k then finds its segment and stores row k.
// Every store is one 32-bit word per lane and instruction (put32, for vehicle.hip's reason).  No atomics, no traffic between
// workgroups: the same inputs give the same bits on every launch.
#include "sched.h"

#pragma clang fp contract(off)

namespace adx {

namespace {

constexpr int kExMaxScenes = 65535, kExMaxWindow = 32, kExMaxSlots = 64, kExMaxPlanes = 8, kExMaxHorizon = 64, kExMaxDim = 16;
constexpr int kExDisc = 64, kExPlane = 128, kExEnd = 136;      // leader codes: 0..63 a box, then these
constexpr int kExInfo = 8;

struct ExArgs {
  const float* window;        // [S][R][2]
  const float* velocity;      // [S]
  const float* boxes;         // [S][N][8] or null
  const float* discs;         // [S][M][5] or null
  const float* planes;        // [S][K][3] or null
  float* plan;                // [S][H][D]
  int32_t* leader;            // [S]
  float* info;                // [S][8]
  int R, N, M, K, H, D;
  double xy_scale, waypoint_dt, desired_v, accel, brake, brake_max, headway, jam, gap_min, corridor_half, lat_accel, look_time,
      ego_front, end_margin, look_min;
};

struct ExPath {      // a scene's window in LDS, metres
  double px[kExMaxWindow], py[kExMaxWindow], cum[kExMaxWindow];
  double ex[kExMaxWindow], ey[kExMaxWindow], l2[kExMaxWindow], len[kExMaxWindow], tx[kExMaxWindow], ty[kExMaxWindow];
  int good[kExMaxWindow];
};

struct ExProj {
  double s, d, cx, cy;
  int j;
};

// one 32-bit word per lane and store instruction: volatile keeps the compiler from merging neighbours into a wide store
__device__ __forceinline__ void put32(void* base, size_t word, uint32_t v) { reinterpret_cast<volatile uint32_t*>(base)[word] = v; }

// "each word is rounded to fp32 once; a NaN is stored as 0x7fc00000"
__device__ __forceinline__ uint32_t word32(double v) {
  const float f = (float)v;
  return f != f ? 0x7fc00000u : __builtin_bit_cast(uint32_t, f);
}

// "project" of expert v1: traffic v1's rule over all the segments of the window
__device__ __forceinline__ ExProj project(const ExPath& sp, int R, double qx, double qy) {
  ExProj o = {0.0, __builtin_inf(), 0.0, 0.0, 0};
  for (int j = 0; j < R - 1; ++j) {
    const double ax = sp.px[j], ay = sp.py[j], ex = sp.ex[j], ey = sp.ey[j];
    double t = 0.0;
    if (sp.good[j] != 0) {
      const double rx = qx - ax, ry = qy - ay;
      const double m0 = rx * ex, m1 = ry * ey;
      const double f = (m0 + m1) / sp.l2[j];
      t = f > 0.0 ? (f < 1.0 ? f : 1.0) : 0.0;      // a NaN becomes 0
      if (j == 0 && f < 0.0) t = f;                 // the path begins with a ray: segment 0 is not clamped below
    }
    const double ox = t * ex, oy = t * ey;
    const double cx = ax + ox, cy = ay + oy;
    const double dx = qx - cx, dy = qy - cy;
    const double dxx = dx * dx, dyy = dy * dy;
    const double dd = sqrt(dxx + dyy);
    const double d = dd != dd ? __builtin_inf() : dd;
    if (j == 0 || d < o.d) {      // the lower j on a tie
      const double along = t * sp.len[j];
      o.s = sp.cum[j] + along;
      o.d = d;
      o.cx = cx;
      o.cy = cy;
      o.j = j;
    }
  }
  return o;
}

__global__ void __launch_bounds__(64) expert_plan_kernel(const ExArgs a) {
  __shared__ ExPath sp;
  const int s = blockIdx.x, lane = threadIdx.x, R = a.R;
  // ---- the path ----
  if (lane < R) {
    const float* w = a.window + ((size_t)s * R + lane) * 2;
    sp.px[lane] = (double)w[0] * a.xy_scale;
    sp.py[lane] = (double)w[1] * a.xy_scale;
  }
  __syncthreads();
  if (lane < R - 1) {
    const double ex = sp.px[lane + 1] - sp.px[lane], ey = sp.py[lane + 1] - sp.py[lane];
    const double exx = ex * ex, eyy = ey * ey;
    const double l2 = exx + eyy;
    const bool good = l2 > 0.0;
    const double len = good ? sqrt(l2) : 0.0;
    sp.ex[lane] = ex;
    sp.ey[lane] = ey;
    sp.l2[lane] = l2;
    sp.len[lane] = len;
    sp.tx[lane] = good ? ex / len : 0.0;
    sp.ty[lane] = good ? ey / len : 0.0;
    sp.good[lane] = good ? 1 : 0;
  }
  __syncthreads();
  if (lane == 0) {
    double c = 0.0;
    sp.cum[0] = 0.0;
    for (int j = 0; j < R - 1; ++j) {
      c = c + sp.len[j];
      sp.cum[j + 1] = c;
    }
  }
  __syncthreads();
  const double vin = (double)a.velocity[s];
  const double v0 = vin > 0.0 ? vin : 0.0;
  const ExProj e = project(sp, R, 0.0, 0.0);      // the same in every lane

  // ---- the candidates of this lane, in the contract's order ----
  double best_r = __builtin_inf(), best_u = 0.0;
  int code = -1;
  if (lane < a.N) {
    const float* g = a.boxes + ((size_t)s * a.N + lane) * 8;
    const float fl = g[6], fw = g[7];
    if (fl > 0.f && fw > 0.f) {
      const double cx = (double)g[0] * a.xy_scale, cy = (double)g[1] * a.xy_scale;
      const double vx = ((double)g[2] * a.xy_scale) / a.waypoint_dt, vy = ((double)g[3] * a.xy_scale) / a.waypoint_dt;
      const double hx = (double)g[4], hy = (double)g[5];
      const double hl = ((double)fl * a.xy_scale) / 2.0, hw = ((double)fw * a.xy_scale) / 2.0;
      const ExProj p = project(sp, R, cx, cy);
      const double tx = sp.tx[p.j], ty = sp.ty[p.j];
      const double d0 = hx * tx, d1 = hy * ty;
      const double c0 = hx * ty, c1 = hy * tx;
      const double dt_ = __builtin_fabs(d0 + d1), cr = __builtin_fabs(c0 - c1);
      const double l0 = hl * dt_, l1 = hw * cr;
      const double lon = l0 + l1;
      const double w0 = hl * cr, w1 = hw * dt_;
      const double lat = w0 + w1;
      const double ahead = p.s - e.s;
      if (p.d <= a.corridor_half + lat && ahead > 0.0) {
        const double r = (ahead - lon) - a.ego_front;
        const double u0 = vx * tx, u1 = vy * ty;
        const double us = u0 + u1;
        if (r < best_r) {
          best_r = r;
          best_u = us > 0.0 ? us : 0.0;
          code = lane;
        }
      }
    }
  }
  if (lane < a.M) {
    const float* g = a.discs + ((size_t)s * a.M + lane) * 5;
    const float fr = g[4];
    if (fr > 0.f) {
      const double cx = (double)g[0] * a.xy_scale, cy = (double)g[1] * a.xy_scale;
      const double vx = ((double)g[2] * a.xy_scale) / a.waypoint_dt, vy = ((double)g[3] * a.xy_scale) / a.waypoint_dt;
      const double rad = (double)fr * a.xy_scale;
      const ExProj p = project(sp, R, cx, cy);
      const double tx = sp.tx[p.j], ty = sp.ty[p.j];
      const double ahead = p.s - e.s;
      if (p.d <= a.corridor_half + rad && ahead > 0.0) {
        const double r = (ahead - rad) - a.ego_front;
        const double u0 = vx * tx, u1 = vy * ty;
        const double us = u0 + u1;
        if (r < best_r) {
          best_r = r;
          best_u = us > 0.0 ? us : 0.0;
          code = kExDisc + lane;
        }
      }
    }
  }
  if (lane < a.K) {
    const float* g = a.planes + ((size_t)s * a.K + lane) * 3;
    const double nx = (double)g[0], ny = (double)g[1];
    const double bm = (double)g[2] * a.xy_scale;
    const double beyond = -bm;
    if (!(nx == 0.0 && ny == 0.0) && !(beyond > 0.0)) {
      double ax = e.cx, ay = e.cy, arc_a = e.s;
      const double g0 = nx * ax, g1 = ny * ay;
      double ga = (g0 + g1) - bm, arc = 0.0;
      bool found = false;
      for (int j = 0; j < R - 1; ++j) {
        if (j < e.j) continue;      // uniform: e is
        const double bx = sp.px[j + 1], by = sp.py[j + 1], arc_b = sp.cum[j + 1];
        const double h0 = nx * bx, h1 = ny * by;
        const double gb = (h0 + h1) - bm;
        if (!found && ga <= 0.0 && gb > 0.0) {
          const double fr = ga / (ga - gb);
          const double span = arc_b - arc_a;
          const double part = fr * span;
          arc = arc_a + part;
          found = true;
        }
        ax = bx; ay = by; arc_a = arc_b; ga = gb;
      }
      if (found) {
        const double r = (arc - e.s) - a.ego_front;
        if (r < best_r) {
          best_r = r;
          best_u = 0.0;
          code = kExPlane + lane;
        }
      }
    }
  }
  if (sp.good[R - 2] == 0) {      // the path ends: the same candidate in every lane
    const double r = ((sp.cum[R - 1] - e.s) - a.ego_front) - a.end_margin;
    if (r < best_r) {
      best_r = r;
      best_u = 0.0;
      code = kExEnd;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double orr = __shfl_xor(best_r, off, 64), ou = __shfl_xor(best_u, off, 64);
    const int oc = __shfl_xor(code, off, 64);
    if (orr < best_r || (orr == best_r && oc < code)) {
      best_r = orr;
      best_u = ou;
      code = oc;
    }
  }

  // ---- the curve limit: lane i vertex i ----
  const double lt = v0 * a.look_time;
  const double look = a.look_min + lt;
  double lim = __builtin_inf();
  if (lane >= 1 && lane <= R - 2 && sp.good[lane - 1] != 0 && sp.good[lane] != 0) {
    const double ah = sp.cum[lane] - e.s;
    if (ah >= 0.0 && ah <= look) {
      const double chx = sp.px[lane + 1] - sp.px[lane - 1], chy = sp.py[lane + 1] - sp.py[lane - 1];
      const double cxx = chx * chx, cyy = chy * chy;
      const double lc = sqrt(cxx + cyy);
      const double x0 = sp.ex[lane - 1] * sp.ey[lane], x1 = sp.ey[lane - 1] * sp.ex[lane];
      const double x = __builtin_fabs(x0 - x1);
      const double num = 2.0 * x;
      const double ll = sp.len[lane - 1] * sp.len[lane];
      const double den = ll * lc;
      const double kappa = num / den;
      if (kappa > 0.0) {
        const double q = a.lat_accel / kappa;
        lim = sqrt(q);
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ol = __shfl_xor(lim, off, 64);
    if (ol < lim) lim = ol;
  }
  const double desired = lim < a.desired_v ? lim : a.desired_v;

  // ---- the law, rolled out in every lane; lane k keeps a_k ----
  const double ab = a.accel * a.brake;
  const double den2 = 2.0 * sqrt(ab);
  double v = v0, arc = 0.0, mine = 0.0, acc0 = 0.0;
  for (int k = 0; k < a.H; ++k) {
    if (k == lane) mine = arc;
    const double f = v / desired;
    const double f2 = f * f;
    const double f4 = f2 * f2;
    const double free_ = 1.0 - f4;
    double inter = 0.0;
    if (code >= 0) {
      const double tk = (double)k * a.waypoint_dt;
      const double mv = best_u * tk;
      const double rk = best_r + mv;
      const double gap = rk - arc;
      const double t0 = v * a.headway;
      const double dv = v - best_u;
      const double t1 = v * dv;
      const double t2 = t1 / den2;
      const double dyn = t0 + t2;
      const double star = a.jam + (dyn > 0.0 ? dyn : 0.0);
      const double g = gap > a.gap_min ? gap : a.gap_min;
      const double ratio = star / g;
      inter = ratio * ratio;
    }
    double acc = a.accel * (free_ - inter);
    if (acc < -a.brake_max) acc = -a.brake_max;
    if (acc > a.accel) acc = a.accel;
    if (k == 0) acc0 = acc;
    const double dvv = acc * a.waypoint_dt;
    const double v1 = v + dvv;
    v = v1 > 0.0 ? v1 : 0.0;
    const double ds = v * a.waypoint_dt;
    arc = arc + ds;
  }

  // ---- row `lane` ----
  if (lane < a.H) {
    const double A = e.s + mine;
    int sel = -1, first = -1;
    for (int j = 0; j < R - 1; ++j) {
      if (sp.good[j] == 0) continue;
      if (first < 0) first = j;
      if (sp.cum[j] <= A) sel = j;
    }
    if (sel < 0) sel = first;
    double x = sp.px[0], y = sp.py[0];
    if (sel >= 0) {
      const double al = A - sp.cum[sel];
      const double ox = al * sp.tx[sel], oy = al * sp.ty[sel];
      x = sp.px[sel] + ox;
      y = sp.py[sel] + oy;
    }
    float* o = a.plan + ((size_t)s * a.H + lane) * a.D;
    put32(o, 0, word32(x / a.xy_scale));
    put32(o, 1, word32(y / a.xy_scale));
    for (int d = 2; d < a.D; ++d) put32(o, d, 0u);
  }
  if (lane < kExInfo) {
    double w = e.s;
    if (lane == 1) w = e.d;
    if (lane == 2) w = desired;
    if (lane == 3) w = best_r;
    if (lane == 4) w = best_u;
    if (lane == 5) w = acc0;
    if (lane == 6) w = v;
    if (lane == 7) w = arc;
    put32(a.info, (size_t)s * kExInfo + lane, word32(w));
  }
  if (lane == 0) put32(a.leader, (size_t)s, (uint32_t)code);
}

bool finite_pos(double v) { return v > 0.0 && v < __builtin_inf(); }
bool finite_nonneg(double v) { return v >= 0.0 && v < __builtin_inf(); }

}  // namespace

int expert_plan(const adx_expert_cfg* c, const float* window, const float* velocity, const float* boxes, const float* discs,
                const float* planes, float* plan, int32_t* leader, float* info, hipStream_t s) {
  ADX_REQUIRE(c != nullptr, "expert plan: null configuration");
  const int S = c->scenes, R = c->window, N = c->n_boxes, M = c->n_discs, K = c->n_planes, H = c->horizon, D = c->dim;
  ADX_REQUIRE(S >= 1 && S <= kExMaxScenes, "expert plan: %d scenes, supported 1..%d", S, kExMaxScenes);
  ADX_REQUIRE(R >= 2 && R <= kExMaxWindow, "expert plan: %d window points, supported 2..%d", R, kExMaxWindow);
  ADX_REQUIRE(N >= 0 && N <= kExMaxSlots, "expert plan: %d boxes, supported 0..%d", N, kExMaxSlots);
  ADX_REQUIRE(M >= 0 && M <= kExMaxSlots, "expert plan: %d discs, supported 0..%d", M, kExMaxSlots);
  ADX_REQUIRE(K >= 0 && K <= kExMaxPlanes, "expert plan: %d planes, supported 0..%d", K, kExMaxPlanes);
  ADX_REQUIRE(H >= 2 && H <= kExMaxHorizon, "expert plan: horizon %d, supported 2..%d", H, kExMaxHorizon);
  ADX_REQUIRE(D >= 2 && D <= kExMaxDim, "expert plan: dim %d, supported 2..%d", D, kExMaxDim);
  const double pos[12] = {c->xy_scale, c->waypoint_dt, c->desired_v, c->accel, c->brake, c->brake_max, c->headway, c->jam, c->gap_min,
                          c->corridor_half, c->lat_accel, c->look_time};
  const char* const pos_names[12] = {"xy_scale", "waypoint_dt", "desired_v", "accel", "brake", "brake_max", "headway", "jam", "gap_min",
                                     "corridor_half", "lat_accel", "look_time"};
  for (int i = 0; i < 12; ++i) ADX_REQUIRE(finite_pos(pos[i]), "expert plan: %s %g must be finite and > 0", pos_names[i], pos[i]);
  const double non[3] = {c->ego_front, c->end_margin, c->look_min};
  const char* const non_names[3] = {"ego_front", "end_margin", "look_min"};
  for (int i = 0; i < 3; ++i) ADX_REQUIRE(finite_nonneg(non[i]), "expert plan: %s %g must be finite and >= 0", non_names[i], non[i]);
  ADX_REQUIRE(window != nullptr, "expert plan: null window");
  ADX_REQUIRE(velocity != nullptr, "expert plan: null velocity");
  ADX_REQUIRE((boxes != nullptr) == (N > 0), "expert plan: boxes must be given exactly when n_boxes > 0 (%d)", N);
  ADX_REQUIRE((discs != nullptr) == (M > 0), "expert plan: discs must be given exactly when n_discs > 0 (%d)", M);
  ADX_REQUIRE((planes != nullptr) == (K > 0), "expert plan: planes must be given exactly when n_planes > 0 (%d)", K);
  ADX_REQUIRE(plan != nullptr, "expert plan: null plan");
  ADX_REQUIRE(leader != nullptr, "expert plan: null leader");
  ADX_REQUIRE(info != nullptr, "expert plan: null info");
  const ByteSpan ins[5] = {{window, (size_t)S * R * 2 * sizeof(float)},
                           {velocity, (size_t)S * sizeof(float)},
                           {boxes, (size_t)S * N * 8 * sizeof(float)},
                           {discs, (size_t)S * M * 5 * sizeof(float)},
                           {planes, (size_t)S * K * 3 * sizeof(float)}};
  const char* const in_names[5] = {"window", "velocity", "boxes", "discs", "planes"};
  const ByteSpan outs[3] = {{plan, (size_t)S * H * D * sizeof(float)}, {leader, (size_t)S * sizeof(int32_t)}, {info, (size_t)S * kExInfo * sizeof(float)}};
  const char* const names[3] = {"plan", "leader", "info"};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 5; ++j)
      ADX_REQUIRE(ins[j].p == nullptr || !byte_ranges_overlap(outs[i].p, outs[i].n, ins[j].p, ins[j].n), "expert plan: %s aliases %s",
                  names[i], in_names[j]);
    for (int j = 0; j < i; ++j)
      ADX_REQUIRE(!byte_ranges_overlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n), "expert plan: %s and %s alias each other", names[j],
                  names[i]);
  }
  ExArgs a = {};
  a.window = window; a.velocity = velocity; a.boxes = boxes; a.discs = discs; a.planes = planes;
  a.plan = plan; a.leader = leader; a.info = info;
  a.R = R; a.N = N; a.M = M; a.K = K; a.H = H; a.D = D;
  a.xy_scale = c->xy_scale; a.waypoint_dt = c->waypoint_dt; a.desired_v = c->desired_v; a.accel = c->accel; a.brake = c->brake;
  a.brake_max = c->brake_max; a.headway = c->headway; a.jam = c->jam; a.gap_min = c->gap_min; a.corridor_half = c->corridor_half;
  a.lat_accel = c->lat_accel; a.look_time = c->look_time; a.ego_front = c->ego_front; a.end_margin = c->end_margin;
  a.look_min = c->look_min;
  expert_plan_kernel<<<dim3(S), dim3(64), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

}  // namespace adx
