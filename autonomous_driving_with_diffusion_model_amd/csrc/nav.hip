// What feeds a tick (include/adx.h: "ego frame v1", "route planner v1"): the reference's RoutePlanner.run_step
// (e2e_driving/planner.py:55-92), its world-to-ego rotation of the target point (interact.py:185-202), the route ahead
// (interact.py:174-183), agent_to_world (interact.py:249-260) and the odometry a warm start and a commit take, for every scene of a
// launch and without a host decision.
//
// Everything here is fp64 and latency-bound: a launch moves a few hundred bytes per scene, so the kernels are plain code and the
// only structure is who does what.
//   nav_step_kernel   one workgroup of one wave per scene.  The reference's loop is sequential in three places -- the running
//                     length `cum`, the stop once it exceeds max_distance, the strict running maximum `far` -- and parallel in the
//                     two square roots per point, which are the cost.  So lanes take 64 route points at a time: every lane forms
//                     its segment length and its distance to the ego; the prefix is then added in index order by a uniform loop
//                     over the lanes' segment lengths (the sums the reference forms, in its order, and the stop at the same
//                     point); one butterfly over (d, index) gives the chunk's first largest candidate, which replaces the carried
//                     `far` exactly when the sequential loop would have replaced it.  Then lanes 0 .. R-1 transform the window,
//                     lane 0 the target and the motion, and lanes 0 .. 7 write one word of the next state each.
//   world_to_ego_kernel, ego_to_world_kernel   one thread per record.
// No atomics, no traffic between workgroups: the same input and state give the same bits on every launch.
#include "sched.h"

#pragma clang fp contract(off)

namespace adx {

namespace {

constexpr int kNavMaxPoints = 65536, kNavMaxWindow = 32, kNavMaxScenes = 65535;
constexpr double kHalfPi = 1.57079632679489661923, kPi = 3.14159265358979323846;

struct NavState {      // 32 bytes per scene; all zero = a fresh walk
  int32_t head, valid;
  double px, py, compass;
};
static_assert(sizeof(NavState) == 32, "route planner v1: 32 bytes of state per scene");

// "frame" of ego frame v1
struct Frame {
  double px, py, c, s;
};

__device__ __forceinline__ Frame frame_of(double px, double py, double compass) {
  const double th = compass + kHalfPi;
  return {px, py, cos(th), sin(th)};
}

__device__ __forceinline__ Frame frame_at(const double* pose) {
  const double compass = pose[2];
  return frame_of(pose[0], pose[1], compass != compass ? 0.0 : compass);
}

// "rotate": the ego vector (r1, -r0) of a world vector
__device__ __forceinline__ void rotate(const Frame& f, double dx, double dy, double& ex, double& ey) {
  const double a0 = f.c * dx, a1 = f.s * dy;
  const double r0 = a0 + a1;
  const double b0 = f.s * dx, b1 = f.c * dy;
  const double r1 = -b0 + b1;
  ex = r1;
  ey = -r0;
}

// "point"
__device__ __forceinline__ void to_ego(const Frame& f, double X, double Y, double xy_scale, float& x, float& y) {
  double ex, ey;
  rotate(f, X - f.px, Y - f.py, ex, ey);
  x = (float)(ex / xy_scale);
  y = (float)(ey / xy_scale);
}

__device__ __forceinline__ double norm2(double x, double y) {
  const double xx = x * x, yy = y * y;
  return sqrt(xx + yy);
}

struct NavArgs {
  const double* route;      // [S][G][2]
  const int32_t* cmd;       // [S][G]
  const int32_t* len;       // [S]
  const double* pose;       // [S][3]
  NavState* state;          // [S]
  float* target;            // [S][2]
  int32_t* command;         // [S]
  float* window;            // [S][R][2]
  float* motion;            // [S][3]
  int32_t* fresh;           // [S]
  int32_t* head_out;        // [S]
  int G, R, first;
  double min_distance, max_distance, xy_scale;
};

__global__ void __launch_bounds__(64) nav_step_kernel(const NavArgs a) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const double* route = a.route + (size_t)s * a.G * 2;
  // the state and the inputs, read before anything of the scene is written
  const NavState st = a.state[s];
  int len = a.len[s];
  len = len < 1 ? 1 : (len > a.G ? a.G : len);
  int head = st.head < 0 ? 0 : (st.head > len - 1 ? len - 1 : st.head);
  const double px = a.pose[(size_t)s * 3 + 0], py = a.pose[(size_t)s * 3 + 1];
  const Frame f = frame_at(a.pose + (size_t)s * 3);
  const int n = len - head;

  int next = head;
  if (n > 1) {
    double cum = 0.0, far = -__builtin_inf();
    int to_pop = 0;
    bool stopped = false;
    for (int base = 1; base < n && !stopped; base += 64) {
      const int cnt = n - base < 64 ? n - base : 64;      // points of this chunk: i = base + lane, lane < cnt
      double seg = 0.0, d = 0.0;
      if (lane < cnt) {
        const double* b = route + (size_t)(head + base + lane) * 2;      // head + i <= len - 1
        const double bx = b[0], by = b[1];
        seg = norm2(bx - b[-2], by - b[-1]);
        d = norm2(bx - px, by - py);
      }
      // the prefix in index order: uniform, every lane forms the same sums
      int visited = cnt;
      for (int j = 0; j < cnt; ++j) {
        if (cum > a.max_distance) {
          visited = j;
          stopped = true;
          break;
        }
        cum = cum + __shfl(seg, j, 64);
      }
      const bool cand = lane < visited && d <= a.min_distance && d > far;
      double v = cand ? d : -__builtin_inf();
      int idx = lane;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(idx, off, 64);
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
      }
      if (v > far) {      // some lane was a candidate: the first of the largest
        far = v;
        to_pop = base + idx;
      }
    }
    const int keep = n - 2;      // n >= 2
    head += to_pop < keep ? to_pop : keep;
    next = head + 1;              // <= len - 1: at least two points remain
  }

  if (lane < a.R) {
    int i = head + a.first + lane;
    i = i > len - 1 ? len - 1 : i;
    float x, y;
    to_ego(f, route[(size_t)i * 2], route[(size_t)i * 2 + 1], a.xy_scale, x, y);
    float* w = a.window + ((size_t)s * a.R + lane) * 2;
    w[0] = x;
    w[1] = y;
  }
  if (lane == 0) {
    float x, y;
    to_ego(f, route[(size_t)next * 2], route[(size_t)next * 2 + 1], a.xy_scale, x, y);
    a.target[(size_t)s * 2 + 0] = x;
    a.target[(size_t)s * 2 + 1] = y;
    a.command[s] = a.cmd[(size_t)s * a.G + next];
    a.head_out[s] = head;
    const double compass = a.pose[(size_t)s * 3 + 2] != a.pose[(size_t)s * 3 + 2] ? 0.0 : a.pose[(size_t)s * 3 + 2];
    float tx = 0.f, ty = 0.f, phi = 0.f;
    if (st.valid != 0) {
      to_ego(frame_of(st.px, st.py, st.compass), px, py, a.xy_scale, tx, ty);
      const double d = compass - st.compass;
      const double turns = ceil((d - kPi) / (2.0 * kPi));
      const double back = (2.0 * kPi) * turns;
      phi = (float)(d - back);
    }
    a.motion[(size_t)s * 3 + 0] = tx;
    a.motion[(size_t)s * 3 + 1] = ty;
    a.motion[(size_t)s * 3 + 2] = phi;
    a.fresh[s] = st.valid != 0 ? 0 : 1;
  }
  // the next state, one 32-bit word per lane: head, valid = 1, then this tick's pose with the compass as used
  if (lane < 8) {
    const double c2 = a.pose[(size_t)s * 3 + 2];
    const double field = lane < 4 ? px : (lane < 6 ? py : (c2 != c2 ? 0.0 : c2));
    const unsigned long long bits = __builtin_bit_cast(unsigned long long, field);
    const uint32_t half = (lane & 1) != 0 ? (uint32_t)(bits >> 32) : (uint32_t)bits;
    reinterpret_cast<uint32_t*>(a.state + s)[lane] = lane == 0 ? (uint32_t)head : (lane == 1 ? 1u : half);
  }
}

__global__ void __launch_bounds__(256) nav_reset_kernel(NavState* state, const uint8_t* mask, int scenes) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= scenes) return;
  if (mask == nullptr || mask[s] != 0) state[s] = NavState{0, 0, 0.0, 0.0, 0.0};
}

constexpr int kEgoWidthIn[4] = {2, 5, 3, 7}, kEgoWidthOut[4] = {2, 5, 3, 8};

__global__ void __launch_bounds__(256) world_to_ego_kernel(int kind, const double* in, const double* pose, float* out, int scenes, int n,
                                                           double xy_scale, double vel_scale) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;      // scenes * n <= 65535 * 65536: fits 32 bits unsigned
  if (i >= (unsigned)scenes * (unsigned)n) return;
  const unsigned s = i / (unsigned)n;
  const Frame f = frame_at(pose + (size_t)s * 3);
  if (kind == ADX_EGO_POINTS) {
    const double* p = in + (size_t)i * 2;
    float x, y;
    to_ego(f, p[0], p[1], xy_scale, x, y);
    out[(size_t)i * 2 + 0] = x;
    out[(size_t)i * 2 + 1] = y;
  } else if (kind == ADX_EGO_DISCS) {
    const double* p = in + (size_t)i * 5;
    float* o = out + (size_t)i * 5;
    double vx, vy;
    to_ego(f, p[0], p[1], xy_scale, o[0], o[1]);
    rotate(f, p[2], p[3], vx, vy);
    o[2] = (float)(vx * vel_scale);
    o[3] = (float)(vy * vel_scale);
    o[4] = (float)(p[4] / xy_scale);
  } else if (kind == ADX_EGO_PLANES) {
    const double* p = in + (size_t)i * 3;
    float* o = out + (size_t)i * 3;
    double nx, ny;
    rotate(f, p[0], p[1], nx, ny);
    const double t0 = p[0] * f.px, t1 = p[1] * f.py;
    const double off = t0 + t1;
    o[0] = (float)nx;
    o[1] = (float)ny;
    o[2] = (float)((p[2] - off) / xy_scale);
  } else {
    const double* p = in + (size_t)i * 7;
    float* o = out + (size_t)i * 8;
    double vx, vy, ux, uy;
    to_ego(f, p[0], p[1], xy_scale, o[0], o[1]);
    rotate(f, p[2], p[3], vx, vy);
    rotate(f, cos(p[4]), sin(p[4]), ux, uy);
    o[2] = (float)(vx * vel_scale);
    o[3] = (float)(vy * vel_scale);
    o[4] = (float)ux;
    o[5] = (float)uy;
    o[6] = (float)(p[5] / xy_scale);
    o[7] = (float)(p[6] / xy_scale);
  }
}

__global__ void __launch_bounds__(256) ego_to_world_kernel(const float* plans, const double* pose, double* out, int rows, int scenes,
                                                           int H, int D, double xy_scale) {
  const int i = blockIdx.x * 256 + threadIdx.x;      // rows * H <= 2^30
  if (i >= rows * H) return;
  const int r = i / H;
  const Frame f = frame_at(pose + (size_t)(r % scenes) * 3);
  const float* p = plans + (size_t)i * D;
  const double a0 = -((double)p[1] * xy_scale), a1 = (double)p[0] * xy_scale;
  const double m0 = f.c * a0, m1 = f.s * a1;
  const double n0 = f.s * a0, n1 = f.c * a1;
  out[(size_t)i * 2 + 0] = (m0 - m1) + f.px;
  out[(size_t)i * 2 + 1] = (n0 + n1) + f.py;
}

bool finite_pos(double v) { return v > 0.0 && v < __builtin_inf(); }

}  // namespace

size_t nav_state_bytes(int scenes) { return scenes >= 1 && scenes <= kNavMaxScenes ? (size_t)scenes * sizeof(NavState) : 0; }

int nav_reset(void* state, int scenes, const uint8_t* mask, hipStream_t s) {
  ADX_REQUIRE(scenes >= 1 && scenes <= kNavMaxScenes, "nav reset: %d scenes, supported 1..%d", scenes, kNavMaxScenes);
  ADX_REQUIRE(state != nullptr, "nav reset: null state");
  ADX_REQUIRE(mask == nullptr || !byte_ranges_overlap(state, nav_state_bytes(scenes), mask, (size_t)scenes),
              "nav reset: the mask overlaps the state");
  nav_reset_kernel<<<dim3(ceil_div(scenes, 256)), dim3(256), 0, s>>>(static_cast<NavState*>(state), mask, scenes);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

int nav_step(const adx_nav_cfg* c, const double* route, const int32_t* cmd, const int32_t* len, const double* pose, void* state,
             float* target, int32_t* command, float* window, float* motion, int32_t* fresh, int32_t* head_out, hipStream_t s) {
  ADX_REQUIRE(c != nullptr, "nav step: null configuration");
  const int S = c->scenes, G = c->max_points, R = c->window;
  ADX_REQUIRE(S >= 1 && S <= kNavMaxScenes, "nav step: %d scenes, supported 1..%d", S, kNavMaxScenes);
  ADX_REQUIRE(G >= 1 && G <= kNavMaxPoints, "nav step: %d route points, supported 1..%d", G, kNavMaxPoints);
  ADX_REQUIRE(R >= 2 && R <= kNavMaxWindow, "nav step: a window of %d points, supported 2..%d", R, kNavMaxWindow);
  ADX_REQUIRE(c->first == 0 || c->first == 1, "nav step: first %d, supported 0 or 1", c->first);
  ADX_REQUIRE(finite_pos(c->min_distance), "nav step: min_distance %g must be finite and > 0", c->min_distance);
  ADX_REQUIRE(finite_pos(c->max_distance), "nav step: max_distance %g must be finite and > 0", c->max_distance);
  ADX_REQUIRE(finite_pos(c->xy_scale), "nav step: xy_scale %g must be finite and > 0", c->xy_scale);
  const ByteSpan ins[5] = {{route, (size_t)S * G * 2 * sizeof(double)},
                           {cmd, (size_t)S * G * sizeof(int32_t)},
                           {len, (size_t)S * sizeof(int32_t)},
                           {pose, (size_t)S * 3 * sizeof(double)},
                           {state, nav_state_bytes(S)}};
  const char* const in_names[5] = {"route", "cmd", "len", "pose", "the state"};
  const ByteSpan outs[6] = {{target, (size_t)S * 2 * sizeof(float)},   {command, (size_t)S * sizeof(int32_t)},
                            {window, (size_t)S * R * 2 * sizeof(float)}, {motion, (size_t)S * 3 * sizeof(float)},
                            {fresh, (size_t)S * sizeof(int32_t)},      {head_out, (size_t)S * sizeof(int32_t)}};
  const char* const names[6] = {"target", "command", "window", "motion", "fresh", "head_out"};
  const char* const bare[5] = {"route", "cmd", "len", "pose", "state"};
  for (int j = 0; j < 5; ++j) ADX_REQUIRE(ins[j].p != nullptr, "nav step: null %s", bare[j]);
  for (int i = 0; i < 6; ++i) ADX_REQUIRE(outs[i].p != nullptr, "nav step: null %s", names[i]);
  for (int i = 0; i < 6; ++i) {
    for (int j = 0; j < 5; ++j)
      ADX_REQUIRE(!byte_ranges_overlap(outs[i].p, outs[i].n, ins[j].p, ins[j].n), "nav step: %s aliases %s", names[i], in_names[j]);
    for (int j = 0; j < i; ++j)
      ADX_REQUIRE(!byte_ranges_overlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n), "nav step: %s and %s alias each other", names[j],
                  names[i]);
  }
  for (int j = 0; j < 4; ++j)
    ADX_REQUIRE(!byte_ranges_overlap(ins[4].p, ins[4].n, ins[j].p, ins[j].n), "nav step: the state aliases %s", in_names[j]);
  NavArgs a = {};
  a.route = route; a.cmd = cmd; a.len = len; a.pose = pose;
  a.state = static_cast<NavState*>(state);
  a.target = target; a.command = command; a.window = window; a.motion = motion; a.fresh = fresh; a.head_out = head_out;
  a.G = G; a.R = R; a.first = c->first;
  a.min_distance = c->min_distance; a.max_distance = c->max_distance; a.xy_scale = c->xy_scale;
  nav_step_kernel<<<dim3(S), dim3(64), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

int world_to_ego(int kind, const double* in, const double* pose, float* out, int scenes, int n, double xy_scale, double vel_scale,
                 hipStream_t s) {
  ADX_REQUIRE(kind >= ADX_EGO_POINTS && kind <= ADX_EGO_BOXES, "world to ego: kind %d, supported 0..3", kind);
  ADX_REQUIRE(scenes >= 1 && scenes <= kNavMaxScenes, "world to ego: %d scenes, supported 1..%d", scenes, kNavMaxScenes);
  ADX_REQUIRE(n >= 1 && n <= kNavMaxPoints, "world to ego: %d records per scene, supported 1..%d", n, kNavMaxPoints);
  ADX_REQUIRE(finite_pos(xy_scale), "world to ego: xy_scale %g must be finite and > 0", xy_scale);
  const bool moving = kind == ADX_EGO_DISCS || kind == ADX_EGO_BOXES;
  ADX_REQUIRE(!moving || (vel_scale > -__builtin_inf() && vel_scale < __builtin_inf()), "world to ego: vel_scale %g must be finite",
              vel_scale);
  ADX_REQUIRE(in != nullptr, "world to ego: null in");
  ADX_REQUIRE(pose != nullptr, "world to ego: null pose");
  ADX_REQUIRE(out != nullptr, "world to ego: null out");
  const size_t recs = (size_t)scenes * n, out_bytes = recs * kEgoWidthOut[kind] * sizeof(float);
  ADX_REQUIRE(!byte_ranges_overlap(out, out_bytes, in, recs * kEgoWidthIn[kind] * sizeof(double)), "world to ego: out aliases in");
  ADX_REQUIRE(!byte_ranges_overlap(out, out_bytes, pose, (size_t)scenes * 3 * sizeof(double)), "world to ego: out aliases pose");
  world_to_ego_kernel<<<dim3((unsigned)((recs + 255) / 256)), dim3(256), 0, s>>>(kind, in, pose, out, scenes, n, xy_scale, vel_scale);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

int ego_to_world(const float* plans, const double* pose, double* out, int rows, int scenes, int horizon, int dim, double xy_scale,
                 hipStream_t s) {
  ADX_REQUIRE(scenes >= 1 && scenes <= kNavMaxScenes, "ego to world: %d scenes, supported 1..%d", scenes, kNavMaxScenes);
  ADX_REQUIRE(rows >= 1 && rows % scenes == 0, "ego to world: %d rows, not a positive multiple of %d scenes", rows, scenes);
  ADX_REQUIRE(horizon >= 1 && horizon <= kNavMaxPoints, "ego to world: horizon %d, supported 1..%d", horizon, kNavMaxPoints);
  ADX_REQUIRE(dim >= 2 && dim <= 16, "ego to world: transition dim %d, supported 2..16", dim);
  ADX_REQUIRE((int64_t)rows * horizon <= (int64_t)1 << 30, "ego to world: %d rows of %d waypoints, supported up to 2^30 waypoints", rows,
              horizon);
  ADX_REQUIRE(finite_pos(xy_scale), "ego to world: xy_scale %g must be finite and > 0", xy_scale);
  ADX_REQUIRE(plans != nullptr, "ego to world: null plans");
  ADX_REQUIRE(pose != nullptr, "ego to world: null pose");
  ADX_REQUIRE(out != nullptr, "ego to world: null out");
  const size_t pts = (size_t)rows * horizon, out_bytes = pts * 2 * sizeof(double);
  ADX_REQUIRE(!byte_ranges_overlap(out, out_bytes, plans, pts * dim * sizeof(float)), "ego to world: out aliases plans");
  ADX_REQUIRE(!byte_ranges_overlap(out, out_bytes, pose, (size_t)scenes * 3 * sizeof(double)), "ego to world: out aliases pose");
  ego_to_world_kernel<<<dim3((unsigned)((pts + 255) / 256)), dim3(256), 0, s>>>(plans, pose, out, rows, scenes, horizon, dim, xy_scale);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

}  // namespace adx
