// What makes a drive stop and start again (include/adx.h: "signals v1"): the traffic lights and stop signs of every scene -- which
// stop lines bind the ego at this tick, as the half-planes a guide takes, and the reference's RunRedLight and RunStopSign criteria
// -- advanced by one tick per launch with the records in device memory.
//
// fp64, no contraction, latency-bound like drive.hip, and laid out like it:
//   signals_step_kernel   one workgroup of one wave per scene, lane j owns slot j.  Geometry, phase, gate and crossing are per
//                         slot and run in parallel; a ballot of the emitting lanes and the population count of the bits below a
//                         lane give it its plane slot; the lowest set bit of the gated-stop ballot is a new target; the lowest
//                         set bit of the run ballot is a first infraction's slot.  The record itself is sequential bookkeeping:
//                         lane 0 forms it in LDS, then lanes 0 .. 15 store one 32-bit word of it each (narrow stores, for
//                         vehicle.hip's reason).
//   signals_reset_kernel  one thread per word.
// No atomics, no traffic between workgroups: the same inputs and state give the same bits on every launch.
#include "sched.h"

#pragma clang fp contract(off)

namespace adx {

namespace {

constexpr int kSigMaxScenes = 65535, kSigMaxSlots = 64, kSigMaxPlanes = 8, kSigWords = 16, kSigWidth = 10;
constexpr double kHalfPi = 1.57079632679489661923;
constexpr int kEmpty = 0, kGreen = 1, kYellow = 2, kRed = 3, kSign = 4;

struct SigState {      // 64 bytes per scene; all zero = fresh
  int32_t ticks, have, target, stop_done, red_runs, stop_runs, stops_met, first_tick, first_slot, emitted, flags, pad;
  double qx, qy;
};
static_assert(sizeof(SigState) == 4 * kSigWords, "signals v1: 64 bytes of state per scene");

struct SigArgs {
  const double* signals;      // [S][N][10]
  const double* pose;         // [S][3]
  const float* velocity;      // [S]
  const int32_t* hold;        // [S] or null
  SigState* state;            // [S]
  float* planes;              // [S][P][3]
  int32_t* phase;             // [S][N]
  int N, P, stop_on_yellow;
  double dt, xy_scale, margin, probe, min_cos, speed_threshold;
};

__device__ __forceinline__ void put_plane(float* o, float nx, float ny, float b) {
  o[0] = nx;
  o[1] = ny;
  o[2] = b;
}

__global__ void __launch_bounds__(64) signals_step_kernel(const SigArgs a) {
  __shared__ SigState rec;
  const int s = blockIdx.x, lane = threadIdx.x;
  // the state, read before anything of the scene is written (uniform: every lane holds it)
  const SigState st = a.state[s];
  const bool held = a.hold != nullptr && a.hold[s] != 0;
  const double px = a.pose[(size_t)s * 3 + 0], py = a.pose[(size_t)s * 3 + 1];
  const double c2 = a.pose[(size_t)s * 3 + 2];
  // "frame" of ego frame v1: the same two library calls
  const double th = (c2 != c2 ? 0.0 : c2) + kHalfPi;
  const double c = cos(th), sn = sin(th);
  const double fx = -c, fy = -sn;
  // the clock
  const bool have = st.have != 0;
  const int ticks = have ? st.ticks + 1 : 0;
  const double tm = (double)ticks * a.dt;
  // the probe
  const double e0 = a.probe * fx, e1 = a.probe * fy;
  const double qx = px + e0, qy = py + e1;

  // ---- slot `lane` ----
  bool live = false, is_stop = false, gate = false, beyond = false, run = false;
  int phase = kEmpty;
  double ax = 0.0, ay = 0.0, nx = 0.0, ny = 0.0;
  if (lane < a.N) {
    const double* g = a.signals + ((size_t)s * a.N + lane) * kSigWidth;
    ax = g[0];
    ay = g[1];
    const double kind = g[4], reach = g[5], offset = g[6], green = g[7], yellow = g[8], red = g[9];
    const double dx = g[2] - ax, dy = g[3] - ay;
    const double dxx = dx * dx, dyy = dy * dy;
    const double L = sqrt(dxx + dyy);
    const double gy = green + yellow;
    const double cycle = gy + red;
    const bool is_light = kind == 1.0;
    is_stop = kind == 2.0;
    const bool timed = green >= 0.0 && yellow >= 0.0 && red >= 0.0 && cycle > 0.0;
    live = (is_light || is_stop) && L > 0.0 && reach > 0.0 && (is_stop || timed);
    if (live) {
      const double tx = dx / L, ty = dy / L;
      nx = -ty;
      ny = tx;
      const double rx = px - ax, ry = py - ay;
      const double o0 = nx * rx, o1 = ny * ry;
      const double lon = o0 + o1;
      const double a0 = tx * rx, a1 = ty * ry;
      const double lat = a0 + a1;
      const double h0 = nx * fx, h1 = ny * fy;
      const double head = h0 + h1;
      const bool inside = lat >= 0.0 && lat <= L;
      gate = lon <= 0.0 && lon >= -reach && inside && head > a.min_cos;
      beyond = lon > 0.0 && inside;
      if (is_stop) {
        phase = kSign;
      } else {
        double tau = fmod(tm + offset, cycle);
        if (tau < 0.0) tau = tau + cycle;
        phase = tau < green ? kGreen : (tau < gy ? kYellow : kRed);
      }
      if (have) {
        const double sx = st.qx - ax, sy = st.qy - ay;
        const double p0 = nx * sx, p1 = ny * sy;
        const double l0 = p0 + p1;
        const double ux = qx - ax, uy = qy - ay;
        const double r0 = nx * ux, r1 = ny * uy;
        const double l1 = r0 + r1;
        if (l0 <= 0.0 && l1 > 0.0) {
          const double u = l0 / (l0 - l1);
          const double m00 = tx * sx, m01 = ty * sy;
          const double m0 = m00 + m01;
          const double m10 = tx * ux, m11 = ty * uy;
          const double m1 = m10 + m11;
          const double du = u * (m1 - m0);
          const double mc = m0 + du;
          run = mc >= 0.0 && mc <= L && phase == kRed;
        }
      }
    }
    a.phase[(size_t)s * a.N + lane] = phase;
  }
  float* planes = a.planes + (size_t)s * a.P * 3;
  if (held) {      // frozen: the record stays, every plane is inert
    if (lane < a.P) put_plane(planes + lane * 3, 0.f, 0.f, 1.f);
    return;
  }

  // ---- the red-light runs, then the stop sign machine (uniform: every lane computes it from the ballots) ----
  const unsigned long long run_mask = __ballot(run);
  const unsigned long long stop_mask = __ballot(gate && is_stop);
  int target = st.target, stop_done = st.stop_done, stop_runs = st.stop_runs, stops_met = st.stops_met, stop_slot = -1;
  if (target == 0) {
    if (stop_mask != 0ull) {
      target = __ffsll((long long)stop_mask);      // slot + 1
      stop_done = 0;
      stops_met = stops_met + 1;
    }
  } else {
    if ((double)a.velocity[s] < a.speed_threshold) stop_done = 1;
    const int j = (target - 1) & 63;      // a stored target outside 1..64 cannot index past the wave
    const bool t_gate = __shfl((int)gate, j, 64) != 0, t_beyond = __shfl((int)beyond, j, 64) != 0;
    if (!t_gate) {
      if (t_beyond && stop_done == 0) {
        stop_runs = stop_runs + 1;
        stop_slot = j;
      }
      target = 0;
    }
  }

  // ---- emission, after the machine ----
  const bool emit = gate && (is_stop ? !(lane == target - 1 && stop_done != 0) : (phase == kRed || (phase == kYellow && a.stop_on_yellow != 0)));
  const unsigned long long emit_mask = __ballot(emit);
  const int count = __popcll(emit_mask);
  const int slot = __popcll(emit_mask & ((1ull << lane) - 1ull));      // lane <= 63: the shift is defined
  const int emitted = count < a.P ? count : a.P;
  if (emit && slot < a.P) {
    // ego frame v1, kind 2, of the world plane (n, n . A - margin)
    const double w0 = nx * ax, w1 = ny * ay;
    const double b = (w0 + w1) - a.margin;
    const double k0 = c * nx, k1 = sn * ny;
    const double r0 = k0 + k1;
    const double j0 = sn * nx, j1 = c * ny;
    const double r1 = -j0 + j1;
    const double t0 = nx * px, t1 = ny * py;
    const double off = t0 + t1;
    put_plane(planes + slot * 3, (float)r1, (float)-r0, (float)((b - off) / a.xy_scale));
  }
  if (lane >= emitted && lane < a.P) put_plane(planes + lane * 3, 0.f, 0.f, 1.f);

  // ---- the record: lane 0 ----
  if (lane == 0) {
    SigState n = st;
    n.ticks = ticks;
    n.have = 1;
    n.target = target;
    n.stop_done = stop_done;
    n.red_runs = st.red_runs + __popcll(run_mask);
    n.stop_runs = stop_runs;
    n.stops_met = stops_met;
    if (st.red_runs + st.stop_runs == 0) {      // the first infraction of either kind, a light before the sign
      if (run_mask != 0ull) {
        n.first_tick = ticks;
        n.first_slot = __ffsll((long long)run_mask) - 1;
      } else if (stop_slot >= 0) {
        n.first_tick = ticks;
        n.first_slot = stop_slot;
      }
    }
    n.emitted = emitted;
    n.flags = st.flags | (count > a.P ? 1 : 0);
    n.pad = 0;
    n.qx = qx;
    n.qy = qy;
    rec = n;
  }
  __syncthreads();
  if (lane < kSigWords) reinterpret_cast<uint32_t*>(a.state + s)[lane] = reinterpret_cast<const uint32_t*>(&rec)[lane];
}

__global__ void __launch_bounds__(256) signals_reset_kernel(uint32_t* state, const uint8_t* mask, float* planes, int scenes, int P) {
  const int i = blockIdx.x * 256 + threadIdx.x;      // scenes * 16 < 2^21
  if (i >= scenes * kSigWords) return;
  const int s = i / kSigWords, w = i % kSigWords;
  if (mask != nullptr && mask[s] == 0) return;
  state[i] = 0u;
  if (planes != nullptr && w < P) {
    float* o = planes + ((size_t)s * P + w) * 3;
    put_plane(o, 0.f, 0.f, 1.f);
  }
}

bool finite_pos(double v) { return v > 0.0 && v < __builtin_inf(); }
bool finite_nonneg(double v) { return v >= 0.0 && v < __builtin_inf(); }
bool finite_any(double v) { return v > -__builtin_inf() && v < __builtin_inf(); }

}  // namespace

size_t signals_state_bytes(int scenes) { return scenes >= 1 && scenes <= kSigMaxScenes ? (size_t)scenes * sizeof(SigState) : 0; }

int signals_reset(void* state, int scenes, const uint8_t* mask, float* planes_out, int n_planes, hipStream_t s) {
  ADX_REQUIRE(scenes >= 1 && scenes <= kSigMaxScenes, "signals reset: %d scenes, supported 1..%d", scenes, kSigMaxScenes);
  ADX_REQUIRE(state != nullptr, "signals reset: null state");
  ADX_REQUIRE(planes_out == nullptr || (n_planes >= 1 && n_planes <= kSigMaxPlanes), "signals reset: %d planes, supported 1..%d",
              n_planes, kSigMaxPlanes);
  const size_t nb = signals_state_bytes(scenes), pb = planes_out == nullptr ? 0 : (size_t)scenes * n_planes * 3 * sizeof(float);
  ADX_REQUIRE(mask == nullptr || !byte_ranges_overlap(state, nb, mask, (size_t)scenes), "signals reset: the mask overlaps the state");
  ADX_REQUIRE(planes_out == nullptr || !byte_ranges_overlap(state, nb, planes_out, pb), "signals reset: planes_out overlaps the state");
  ADX_REQUIRE(planes_out == nullptr || mask == nullptr || !byte_ranges_overlap(planes_out, pb, mask, (size_t)scenes),
              "signals reset: the mask overlaps planes_out");
  signals_reset_kernel<<<dim3(ceil_div(scenes * kSigWords, 256)), dim3(256), 0, s>>>(static_cast<uint32_t*>(state), mask, planes_out, scenes,
                                                                                    planes_out == nullptr ? 0 : n_planes);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

int signals_step(const adx_signals_cfg* c, const double* signals, const double* pose, const float* velocity, const int32_t* hold,
                 void* state, float* planes, int32_t* phase, hipStream_t s) {
  ADX_REQUIRE(c != nullptr, "signals step: null configuration");
  const int S = c->scenes, N = c->n_signals, P = c->n_planes;
  ADX_REQUIRE(S >= 1 && S <= kSigMaxScenes, "signals step: %d scenes, supported 1..%d", S, kSigMaxScenes);
  ADX_REQUIRE(N >= 1 && N <= kSigMaxSlots, "signals step: %d signals, supported 1..%d", N, kSigMaxSlots);
  ADX_REQUIRE(P >= 1 && P <= kSigMaxPlanes, "signals step: %d planes, supported 1..%d", P, kSigMaxPlanes);
  ADX_REQUIRE(finite_pos(c->dt), "signals step: dt %g must be finite and > 0", c->dt);
  ADX_REQUIRE(finite_pos(c->xy_scale), "signals step: xy_scale %g must be finite and > 0", c->xy_scale);
  ADX_REQUIRE(finite_nonneg(c->margin), "signals step: margin %g must be finite and >= 0", c->margin);
  ADX_REQUIRE(finite_any(c->probe), "signals step: probe %g must be finite", c->probe);
  ADX_REQUIRE(c->min_cos >= -1.0 && c->min_cos < 1.0, "signals step: min_cos %g must lie in [-1, 1)", c->min_cos);
  ADX_REQUIRE(finite_nonneg(c->speed_threshold), "signals step: speed_threshold %g must be finite and >= 0", c->speed_threshold);
  const ByteSpan ins[4] = {{signals, (size_t)S * N * kSigWidth * sizeof(double)},
                           {pose, (size_t)S * 3 * sizeof(double)},
                           {velocity, (size_t)S * sizeof(float)},
                           {hold, (size_t)S * sizeof(int32_t)}};
  const char* const in_names[4] = {"signals", "pose", "velocity", "hold"};
  const ByteSpan outs[3] = {{state, signals_state_bytes(S)}, {planes, (size_t)S * P * 3 * sizeof(float)}, {phase, (size_t)S * N * sizeof(int32_t)}};
  const char* const names[3] = {"the state", "planes", "phase"};
  for (int j = 0; j < 3; ++j) ADX_REQUIRE(ins[j].p != nullptr, "signals step: null %s", in_names[j]);
  ADX_REQUIRE(state != nullptr, "signals step: null state");
  for (int i = 1; i < 3; ++i) ADX_REQUIRE(outs[i].p != nullptr, "signals step: null %s", names[i]);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 4; ++j)
      ADX_REQUIRE(ins[j].p == nullptr || !byte_ranges_overlap(outs[i].p, outs[i].n, ins[j].p, ins[j].n), "signals step: %s aliases %s",
                  names[i], in_names[j]);
    for (int j = 0; j < i; ++j)
      ADX_REQUIRE(!byte_ranges_overlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n), "signals step: %s and %s alias each other", names[j],
                  names[i]);
  }
  SigArgs a = {};
  a.signals = signals; a.pose = pose; a.velocity = velocity; a.hold = hold;
  a.state = static_cast<SigState*>(state);
  a.planes = planes; a.phase = phase;
  a.N = N; a.P = P; a.stop_on_yellow = c->stop_on_yellow;
  a.dt = c->dt; a.xy_scale = c->xy_scale; a.margin = c->margin; a.probe = c->probe; a.min_cos = c->min_cos;
  a.speed_threshold = c->speed_threshold;
  signals_step_kernel<<<dim3(S), dim3(64), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

}  // namespace adx
