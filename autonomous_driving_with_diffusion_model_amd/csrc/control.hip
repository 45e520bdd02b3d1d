// Device-side controller (include/adx.h: adx_control_step, "control v1"): waypoints -> (throttle, steer, brake), the reference's
// Controller.control_pid (control/controller.py:29-76) + PIDController (control/pid.py) + the agents' post_process_control, for all
// scenes of a tick in one launch.
//
// One wave per scene, four scenes per workgroup; the waves of a workgroup share nothing (no LDS, no barrier), so a scene's
// result cannot depend on which scenes share its launch.  Lane = waypoint for the staging, lane = segment for the two norms:
//   1. lane i holds wp[i] (lane W: the stand-in target when `target` is NULL); lane i < W - 1 takes |wp[i+1] - wp[i]| and the
//      aim key of segment i from its neighbour's waypoint (one shuffle each);
//   2. the desired speed is summed in index order (W - 2 additions, W - 1 broadcasts: W is 4 in the callers);
//   3. the aim index is an xor butterfly over (key, i) pairs, ties to the lower i, keys that do not qualify at +inf;
//   4. lanes 0, 1, 2 take the three headings at once (one atan2f in the instruction stream);
//   5. each PID reads its ring with lane = chronological slot (up to four per lane), reduces with the fixed xor butterfly and
//      lane 0 writes the new sample and the ring position back: plain stores from a vector lane.
// Every product, sum, division and square root is rounded on its own (no contraction), so the bits do not depend on what the
// compiler would fuse.  Latency-sized like select.hip: one short node at the end of the tick's chain.
#include "adx_common.h"

#pragma clang fp contract(off)      // the whole file: the helpers below are part of the contract's arithmetic too

namespace adx {

namespace {

constexpr int kCtlMaxH = 64, kCtlMaxD = 16, kCtlWaves = 4;

struct ControlArgs {
  const float* traj;
  const float* velocity;
  const float* target;     // [scenes][2] or null
  uint32_t* state;
  float* control;
  adx_control_cfg c;
};

__device__ __forceinline__ float clip_nan(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

__device__ __forceinline__ float norm2(float x, float y) { return sqrtf(x * x + y * y); }

__device__ __forceinline__ float heading(float x, float y) {
  constexpr float kHalfPi = 1.57079632679489661923f, kRadToDeg = 57.295779513082320877f;
  return ((kHalfPi - atan2f(y, x)) * kRadToDeg) / 90.f;
}

__device__ __forceinline__ void post_process(int post, float& throttle, float& steer, float& brake) {
  if (post == ADX_CONTROL_POST_NONE) return;
  if (brake < 0.05f) brake = 0.f;
  if (throttle > brake) brake = 0.f;
  if (brake > 0.5f) {
    throttle = 0.f;
    if (post == ADX_CONTROL_POST_INTERACT) { brake = 1.f; steer = 0.f; }
  }
}

// One step of a windowed PID.  `head`: the ring's next slot, i.e. the oldest sample, which this step replaces.  Chronological
// sample j (0 = oldest kept, n - 1 = e) sits in slot (h + 1 + j) % n; the slot that is overwritten is read by nobody.
__device__ __forceinline__ float pid_step(float e, float* ring, uint32_t* head, int n, float kp, float ki, float kd, int lane) {
  const int h = (int)(*head % (uint32_t)n);         // a ring position from foreign bytes still lands inside the ring
  float out = kp * e;
  if (n >= 2) {
    const float previous = ring[(h + n - 1) % n];
    float p = 0.f;
    for (int j = lane; j < n; j += kWave) p += (j == n - 1) ? e : ring[(h + 1 + j) % n];
    const float mean = wave_sum(p) / (float)n;
    out = (out + ki * mean) + kd * (e - previous);
  }
  if (lane == 0) {
    ring[h] = e;
    *head = (uint32_t)((h + 1) % n);
  }
  return out;
}

__global__ void __launch_bounds__(kCtlWaves* kWave) control_step_kernel(const ControlArgs a) {
  const adx_control_cfg& c = a.c;
  const int lane = threadIdx.x & (kWave - 1);
  const int s = blockIdx.x * kCtlWaves + (threadIdx.x >> 6);
  if (s >= c.scenes) return;                       // whole waves leave: the shuffles below always see all 64 lanes
  const int H = c.horizon, D = c.dim, W = c.waypoints;
  const float* row = a.traj + (size_t)s * H * D;
  float* out = a.control + (size_t)s * 3;

  if (c.source == ADX_CONTROL_SOURCE_ACTION) {
    if (lane == 0) {
      float throttle = row[D - 3], steer = row[D - 2], brake = row[D - 1];
      post_process(c.post, throttle, steer, brake);
      out[0] = throttle; out[1] = steer; out[2] = brake;
    }
    return;
  }

  // 1. waypoints; lane W is the stand-in target (W < H then: checked on the host)
  float wx = 0.f, wy = 0.f;
  if (lane < W || (a.target == nullptr && lane == W)) {
    const float* p = row + (size_t)lane * D;
    wx = c.sign_x * (c.xy_scale * p[0]);
    wy = D > 1 ? c.xy_scale * p[1] : 0.f;
  }
  const int next = (lane + 1) & (kWave - 1);
  const float nx = __shfl(wx, next, kWave), ny = __shfl(wy, next, kWave);
  const bool seg = lane < W - 1;
  const float dx = nx - wx, dy = ny - wy;
  const float term = (norm2(dx, dy) * 2.f) / (float)(W - 1);
  const float key = __builtin_fabsf(c.aim_dist - norm2((nx + wx) / 2.f, (ny + wy) / 2.f));

  // 2. desired speed, in index order
  float desired = __shfl(term, 0, kWave);
  for (int i = 1; i < W - 1; ++i) desired += __shfl(term, i, kWave);

  // 3. aim index
  float v = __builtin_inff();
  int idx = lane;
  if (seg && key < __builtin_fabsf(c.aim_dist - 1e5f)) v = key;      // false for a NaN key
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off, kWave);
    const int oi = __shfl_xor(idx, off, kWave);
    if (ov < v || (ov == v && oi < idx)) { v = ov; idx = oi; }
  }
  const float aim_x = __shfl(wx, idx, kWave), aim_y = __shfl(wy, idx, kWave);
  const float last_x = __shfl(dx, W - 2, kWave), last_y = __shfl(dy, W - 2, kWave);
  float tgt_x, tgt_y;
  if (a.target != nullptr) {
    tgt_x = c.sign_x * (c.target_scale * a.target[2 * (size_t)s]);
    tgt_y = c.target_scale * a.target[2 * (size_t)s + 1];
  } else {
    tgt_x = __shfl(wx, W, kWave);
    tgt_y = __shfl(wy, W, kWave);
  }

  // 4. the three headings, one per lane
  const float hx = lane == 0 ? aim_x : (lane == 1 ? last_x : tgt_x);
  const float hy = lane == 0 ? aim_y : (lane == 1 ? last_y : tgt_y);
  const float hd = heading(hx, hy);
  const float angle = __shfl(hd, 0, kWave), angle_last = __shfl(hd, 1, kWave), angle_target = __shfl(hd, 2, kWave);
  const bool to_target = __builtin_fabsf(angle_target) < __builtin_fabsf(angle) ||
                         (__builtin_fabsf(angle_target - angle_last) > c.angle_thresh && tgt_y < c.dist_thresh);

  // 5. the two PIDs on this scene's state
  uint32_t* st = a.state + (size_t)s * (2 + c.n_turn + c.n_speed);
  float* turn_ring = reinterpret_cast<float*>(st + 2);
  float* speed_ring = turn_ring + c.n_turn;
  float steer = clip_nan(pid_step(to_target ? angle_target : angle, turn_ring, st, c.n_turn, c.turn_kp, c.turn_ki, c.turn_kd, lane),
                         -1.f, 1.f);
  const float speed = a.velocity[s];
  const bool braking = desired < c.brake_speed || speed / desired > c.brake_ratio;
  const float delta = clip_nan(desired - speed, 0.f, c.clip_delta);
  const float r = pid_step(delta, speed_ring, st + 1, c.n_speed, c.speed_kp, c.speed_ki, c.speed_kd, lane);
  float throttle = braking ? 0.f : clip_nan(r, 0.f, c.max_throttle);
  float brake = braking ? 1.f : 0.f;
  post_process(c.post, throttle, steer, brake);
  if (lane == 0) { out[0] = throttle; out[1] = steer; out[2] = brake; }
}

__global__ void __launch_bounds__(256) control_reset_kernel(uint32_t* state, const uint8_t* mask, int scenes, int stride) {
  const int i = blockIdx.x * 256 + threadIdx.x;        // scenes * stride <= 65535 * 514: fits
  if (i >= scenes * stride) return;
  if (mask == nullptr || mask[i / stride] != 0) state[i] = 0u;
}

bool windows_ok(int scenes, int n_turn, int n_speed) {
  return scenes >= 1 && scenes <= 65535 && n_turn >= 1 && n_turn <= ADX_CONTROL_MAX_WINDOW && n_speed >= 1 &&
         n_speed <= ADX_CONTROL_MAX_WINDOW;
}

}  // namespace

size_t control_state_bytes(int scenes, int n_turn, int n_speed) {
  return windows_ok(scenes, n_turn, n_speed) ? (size_t)scenes * (2 + n_turn + n_speed) * sizeof(uint32_t) : 0;
}

int control_step(const adx_control_cfg* c, const float* traj, const float* velocity, const float* target, void* state,
                 float* control, hipStream_t s) {
  ADX_REQUIRE(c != nullptr, "control step: null configuration");
  ADX_REQUIRE(c->scenes >= 1 && c->scenes <= 65535, "control step: %d scenes, supported 1..65535", c->scenes);
  ADX_REQUIRE(c->horizon >= 2 && c->horizon <= kCtlMaxH, "control step: horizon %d, supported 2..%d", c->horizon, kCtlMaxH);
  ADX_REQUIRE(c->dim >= 1 && c->dim <= kCtlMaxD, "control step: transition dim %d, supported 1..%d", c->dim, kCtlMaxD);
  ADX_REQUIRE(c->waypoints >= 2 && c->waypoints <= c->horizon, "control step: %d waypoints, supported 2..horizon = %d", c->waypoints,
              c->horizon);
  ADX_REQUIRE(c->n_turn >= 1 && c->n_turn <= ADX_CONTROL_MAX_WINDOW && c->n_speed >= 1 && c->n_speed <= ADX_CONTROL_MAX_WINDOW,
              "control step: window lengths %d and %d, supported 1..%d", c->n_turn, c->n_speed, ADX_CONTROL_MAX_WINDOW);
  ADX_REQUIRE(c->source == ADX_CONTROL_SOURCE_PID || c->source == ADX_CONTROL_SOURCE_ACTION, "control step: unknown source %d", c->source);
  ADX_REQUIRE(c->post >= ADX_CONTROL_POST_NONE && c->post <= ADX_CONTROL_POST_INTERACT, "control step: unknown post %d", c->post);
  ADX_REQUIRE(c->source != ADX_CONTROL_SOURCE_ACTION || c->dim >= 3, "control step: the action source reads the last three of %d columns",
              c->dim);
  ADX_REQUIRE(target != nullptr || c->waypoints < c->horizon,
              "control step: without a target waypoint %d stands in for it, the horizon is %d", c->waypoints, c->horizon);
  ADX_REQUIRE(traj != nullptr && velocity != nullptr && state != nullptr && control != nullptr, "control step: null tensor");
  const size_t traj_bytes = (size_t)c->scenes * c->horizon * c->dim * sizeof(float), vel_bytes = (size_t)c->scenes * sizeof(float);
  const size_t tgt_bytes = target != nullptr ? (size_t)c->scenes * 2 * sizeof(float) : 0, ctl_bytes = (size_t)c->scenes * 3 * sizeof(float);
  const size_t state_bytes = control_state_bytes(c->scenes, c->n_turn, c->n_speed);
  ADX_REQUIRE(!byte_ranges_overlap(control, ctl_bytes, traj, traj_bytes) && !byte_ranges_overlap(control, ctl_bytes, velocity, vel_bytes) &&
                  !(target != nullptr && byte_ranges_overlap(control, ctl_bytes, target, tgt_bytes)) && !byte_ranges_overlap(control, ctl_bytes, state, state_bytes),
              "control step: control overlaps an input or the state");
  ADX_REQUIRE(!byte_ranges_overlap(state, state_bytes, traj, traj_bytes) && !byte_ranges_overlap(state, state_bytes, velocity, vel_bytes) &&
                  !(target != nullptr && byte_ranges_overlap(state, state_bytes, target, tgt_bytes)),
              "control step: the state overlaps an input");
  ControlArgs a;
  a.traj = traj; a.velocity = velocity; a.target = target; a.state = static_cast<uint32_t*>(state); a.control = control;
  a.c = *c;
  control_step_kernel<<<dim3(ceil_div(c->scenes, kCtlWaves)), dim3(kCtlWaves * kWave), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

int control_reset(void* state, int scenes, int n_turn, int n_speed, const uint8_t* mask, hipStream_t s) {
  ADX_REQUIRE(windows_ok(scenes, n_turn, n_speed), "control reset: %d scenes (1..65535), window lengths %d and %d (1..%d)", scenes,
              n_turn, n_speed, ADX_CONTROL_MAX_WINDOW);
  ADX_REQUIRE(state != nullptr, "control reset: null state");
  const int stride = 2 + n_turn + n_speed;
  ADX_REQUIRE(mask == nullptr || !byte_ranges_overlap(state, (size_t)scenes * stride * sizeof(uint32_t), mask, (size_t)scenes),
              "control reset: the mask overlaps the state");
  control_reset_kernel<<<dim3(ceil_div(scenes * stride, 256)), dim3(256), 0, s>>>(static_cast<uint32_t*>(state), mask, scenes, stride);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

}  // namespace adx
