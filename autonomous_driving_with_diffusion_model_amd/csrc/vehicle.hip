// What closes the loop (include/adx.h: "vehicle v1"): a kinematic bicycle that takes a tick's (throttle, steer, brake) to the pose
// the next tick's navigator reads and to the speed its controller reads, for every scene of a launch and without a host decision.
//
// fp64, no contraction, a few dozen operations and 40 bytes of state per scene: latency-bound, so the kernel is plain code.
//   vehicle_step_kernel    one lane per scene, 64 lanes per workgroup.  The sub-steps are sequential by nature (each reads the
//                          speed and the compass the one before it wrote); scenes are independent, so they are the lanes.
//   vehicle_reset_kernel   one lane per scene.
// Every store to the state and to `pose` is one 32-bit word per lane (put64 / put32 below): the state is written through the
// address it was read from, and a wide store whose data registers the next VALU instruction overwrites is the pattern
// tools/check_store_hazard.py exists to catch -- narrow stores cannot form it.
// No atomics, no traffic between lanes: the same control and state give the same bits on every launch.
#include "sched.h"

#pragma clang fp contract(off)

namespace adx {

namespace {

constexpr int kVehMaxScenes = 65535, kVehMaxSubsteps = 16, kVehWords = 10;

struct VehState {      // 40 bytes per scene; all zero = at the origin, at rest, not yet placed
  double x, y, compass, speed;
  int32_t valid, pad;
};
static_assert(sizeof(VehState) == 4 * kVehWords, "vehicle v1: 40 bytes of state per scene");

// one 32-bit word per lane and store instruction: volatile keeps the compiler from merging neighbours into a wide store
__device__ __forceinline__ void put32(void* base, int word, uint32_t v) { reinterpret_cast<volatile uint32_t*>(base)[word] = v; }

__device__ __forceinline__ void put64(void* base, int word, double v) {
  const unsigned long long bits = __builtin_bit_cast(unsigned long long, v);
  put32(base, word, (uint32_t)bits);
  put32(base, word + 1, (uint32_t)(bits >> 32));
}

__device__ __forceinline__ void put_state(VehState* st, double x, double y, double compass, double v, int valid) {
  put64(st, 0, x);
  put64(st, 2, y);
  put64(st, 4, compass);
  put64(st, 6, v);
  put32(st, 8, (uint32_t)valid);
  put32(st, 9, 0u);
}

__device__ __forceinline__ void put_outputs(int s, double x, double y, double compass, double v, double yaw_rate, double* pose,
                                            float* velocity, float* yaw_out) {
  put64(pose + (size_t)s * 3, 0, x);
  put64(pose + (size_t)s * 3, 2, y);
  put64(pose + (size_t)s * 3, 4, compass);
  velocity[s] = (float)v;
  yaw_out[s] = (float)yaw_rate;
}

// "control" of vehicle v1: NaN and inf count as 0, then the clamp, widened exactly
__device__ __forceinline__ double pedal(float c, float lo) {
  const float f = finite_f(c) ? c : 0.f;
  return (double)(f < lo ? lo : (f > 1.f ? 1.f : f));
}

struct VehArgs {
  const float* control;      // [S][3]
  const int32_t* hold;       // [S] or null
  VehState* state;           // [S]
  double* pose;              // [S][3]
  float* velocity;           // [S]
  float* yaw_rate;           // [S]
  int scenes, substeps;
  double sign, dt, h, wheelbase, accel_max, brake_max, drag, roll, v_max, steer_max;
};

__global__ void __launch_bounds__(64) vehicle_step_kernel(const VehArgs a) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= a.scenes) return;
  // the state, read before anything of the scene is written
  const VehState st = a.state[s];
  double x = st.x, y = st.y, compass = st.compass, v = st.speed;
  if (a.hold != nullptr && a.hold[s] != 0) {
    put_outputs(s, x, y, compass, 0.0, 0.0, a.pose, a.velocity, a.yaw_rate);
    put_state(a.state + s, x, y, compass, 0.0, 1);
    return;
  }
  const double throttle = pedal(a.control[(size_t)s * 3 + 0], 0.f);
  const double steer = pedal(a.control[(size_t)s * 3 + 1], -1.f);
  const double brake = pedal(a.control[(size_t)s * 3 + 2], 0.f);
  const double delta = steer * a.steer_max;
  const double k = tan(delta) / a.wheelbase;
  const double c0 = compass;
  const double push = throttle * a.accel_max, pull = brake * a.brake_max;
  for (int i = 0; i < a.substeps; ++i) {
    const double dv = a.drag * v;
    double acc = (push - pull) - dv;
    if (v > 0.0) acc = acc - a.roll;
    const double inc = acc * a.h;
    v = v + inc;
    if (!(v >= 0.0)) v = 0.0;      // negative or NaN
    if (v > a.v_max) v = a.v_max;
    const double sv = a.sign * v;
    const double rate = sv * k;
    const double turn = rate * a.h;
    compass = compass + turn;
    const double dist = v * a.h;
    const double sx = dist * sin(compass), sy = dist * cos(compass);
    x = x + sx;
    y = y - sy;
  }
  const double yaw = (compass - c0) / a.dt;
  put_outputs(s, x, y, compass, v, yaw, a.pose, a.velocity, a.yaw_rate);
  put_state(a.state + s, x, y, compass, v, 1);
}

__global__ void __launch_bounds__(64) vehicle_reset_kernel(VehState* state, int scenes, const double* pose, const double* speed,
                                                           const uint8_t* mask, double* pose_out, float* velocity_out,
                                                           float* yaw_out) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= scenes) return;
  if (mask != nullptr && mask[s] == 0) return;
  double x = 0.0, y = 0.0, compass = 0.0, v = 0.0;
  if (pose != nullptr) {
    x = pose[(size_t)s * 3 + 0];
    y = pose[(size_t)s * 3 + 1];
    compass = pose[(size_t)s * 3 + 2];
    if (compass != compass) compass = 0.0;
    if (speed != nullptr) v = speed[s];
    if (!(v >= 0.0)) v = 0.0;
  }
  if (pose_out != nullptr) put_outputs(s, x, y, compass, v, 0.0, pose_out, velocity_out, yaw_out);
  put_state(state + s, x, y, compass, v, pose != nullptr ? 1 : 0);
}

bool finite_pos(double v) { return v > 0.0 && v < __builtin_inf(); }
bool finite_nonneg(double v) { return v >= 0.0 && v < __builtin_inf(); }

}  // namespace

size_t vehicle_state_bytes(int scenes) { return scenes >= 1 && scenes <= kVehMaxScenes ? (size_t)scenes * sizeof(VehState) : 0; }

int vehicle_reset(void* state, int scenes, const double* pose, const double* speed, const uint8_t* mask, double* pose_out,
                  float* velocity_out, float* yaw_rate_out, hipStream_t s) {
  ADX_REQUIRE(scenes >= 1 && scenes <= kVehMaxScenes, "vehicle reset: %d scenes, supported 1..%d", scenes, kVehMaxScenes);
  ADX_REQUIRE(state != nullptr, "vehicle reset: null state");
  ADX_REQUIRE(pose != nullptr || speed == nullptr, "vehicle reset: a speed without a pose");
  const int n_out = (pose_out != nullptr) + (velocity_out != nullptr) + (yaw_rate_out != nullptr);
  ADX_REQUIRE(n_out == 0 || n_out == 3, "vehicle reset: pose_out, velocity_out and yaw_rate_out come together or not at all");
  const size_t S = (size_t)scenes;
  const ByteSpan ins[3] = {{pose, S * 3 * sizeof(double)}, {speed, S * sizeof(double)}, {mask, S}};
  const char* const in_names[3] = {"pose", "speed", "the mask"};
  const ByteSpan outs[4] = {{state, vehicle_state_bytes(scenes)},
                            {pose_out, S * 3 * sizeof(double)},
                            {velocity_out, S * sizeof(float)},
                            {yaw_rate_out, S * sizeof(float)}};
  const char* const names[4] = {"the state", "pose_out", "velocity_out", "yaw_rate_out"};
  for (int i = 0; i < 4; ++i) {
    if (outs[i].p == nullptr) continue;
    for (int j = 0; j < 3; ++j)
      ADX_REQUIRE(ins[j].p == nullptr || !byte_ranges_overlap(outs[i].p, outs[i].n, ins[j].p, ins[j].n),
                  "vehicle reset: %s overlaps %s", names[i], in_names[j]);
    for (int j = 0; j < i; ++j)
      ADX_REQUIRE(outs[j].p == nullptr || !byte_ranges_overlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n),
                  "vehicle reset: %s and %s alias each other", names[j], names[i]);
  }
  vehicle_reset_kernel<<<dim3(ceil_div(scenes, 64)), dim3(64), 0, s>>>(static_cast<VehState*>(state), scenes, pose, speed, mask, pose_out,
                                                                       velocity_out, yaw_rate_out);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

int vehicle_step(const adx_vehicle_cfg* c, const float* control, const int32_t* hold, void* state, double* pose, float* velocity,
                 float* yaw_rate, hipStream_t s) {
  ADX_REQUIRE(c != nullptr, "vehicle step: null configuration");
  const int S = c->scenes;
  ADX_REQUIRE(S >= 1 && S <= kVehMaxScenes, "vehicle step: %d scenes, supported 1..%d", S, kVehMaxScenes);
  ADX_REQUIRE(c->substeps >= 1 && c->substeps <= kVehMaxSubsteps, "vehicle step: %d substeps, supported 1..%d", c->substeps,
              kVehMaxSubsteps);
  ADX_REQUIRE(c->steer_sign == 1 || c->steer_sign == -1, "vehicle step: steer_sign %d, supported +1 or -1", c->steer_sign);
  ADX_REQUIRE(finite_pos(c->dt), "vehicle step: dt %g must be finite and > 0", c->dt);
  ADX_REQUIRE(finite_pos(c->wheelbase), "vehicle step: wheelbase %g must be finite and > 0", c->wheelbase);
  ADX_REQUIRE(finite_pos(c->accel_max), "vehicle step: accel_max %g must be finite and > 0", c->accel_max);
  ADX_REQUIRE(finite_pos(c->brake_max), "vehicle step: brake_max %g must be finite and > 0", c->brake_max);
  ADX_REQUIRE(finite_pos(c->v_max), "vehicle step: v_max %g must be finite and > 0", c->v_max);
  ADX_REQUIRE(finite_nonneg(c->drag), "vehicle step: drag %g must be finite and >= 0", c->drag);
  ADX_REQUIRE(finite_nonneg(c->roll), "vehicle step: roll %g must be finite and >= 0", c->roll);
  ADX_REQUIRE(c->steer_max > 0.0 && c->steer_max < 1.5, "vehicle step: steer_max %g must lie in (0, 1.5) radians", c->steer_max);
  const ByteSpan ins[3] = {{control, (size_t)S * 3 * sizeof(float)}, {hold, (size_t)S * sizeof(int32_t)}, {state, vehicle_state_bytes(S)}};
  const char* const in_names[3] = {"control", "hold", "the state"};
  const ByteSpan outs[3] = {{pose, (size_t)S * 3 * sizeof(double)}, {velocity, (size_t)S * sizeof(float)}, {yaw_rate, (size_t)S * sizeof(float)}};
  const char* const names[3] = {"pose", "velocity", "yaw_rate"};
  ADX_REQUIRE(control != nullptr, "vehicle step: null control");
  ADX_REQUIRE(state != nullptr, "vehicle step: null state");
  for (int i = 0; i < 3; ++i) ADX_REQUIRE(outs[i].p != nullptr, "vehicle step: null %s", names[i]);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      ADX_REQUIRE(ins[j].p == nullptr || !byte_ranges_overlap(outs[i].p, outs[i].n, ins[j].p, ins[j].n), "vehicle step: %s aliases %s",
                  names[i], in_names[j]);
    for (int j = 0; j < i; ++j)
      ADX_REQUIRE(!byte_ranges_overlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n), "vehicle step: %s and %s alias each other", names[j],
                  names[i]);
  }
  for (int j = 0; j < 2; ++j)
    ADX_REQUIRE(ins[j].p == nullptr || !byte_ranges_overlap(ins[2].p, ins[2].n, ins[j].p, ins[j].n), "vehicle step: the state aliases %s",
                in_names[j]);
  VehArgs a = {};
  a.control = control; a.hold = hold;
  a.state = static_cast<VehState*>(state);
  a.pose = pose; a.velocity = velocity; a.yaw_rate = yaw_rate;
  a.scenes = S; a.substeps = c->substeps;
  a.sign = (double)c->steer_sign; a.dt = c->dt; a.h = c->dt / (double)c->substeps;
  a.wheelbase = c->wheelbase; a.accel_max = c->accel_max; a.brake_max = c->brake_max; a.drag = c->drag; a.roll = c->roll;
  a.v_max = c->v_max; a.steer_max = c->steer_max;
  vehicle_step_kernel<<<dim3(ceil_div(S, 64)), dim3(64), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

}  // namespace adx
