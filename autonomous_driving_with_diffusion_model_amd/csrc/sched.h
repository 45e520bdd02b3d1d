// Entries of sched.hip.  A scheduler step is described by ONE record with named fields and run by ONE function: the exports of
// api.cpp fill a StepCall / DpmCall and step_run / dpm_run validate it, pick the kernel instantiation and launch.
#pragma once
#include "adx_common.h"
#include "guide.h"

namespace adx {

// The guide records of one launch (include/adx.h, "cost guidance v1" to "v5"), each null where the launch has none.  Exports fill
// it, StepCall and DpmCall carry it, guide_cost, traj_select_guide and stop_short take it, and guide_records_check is the one
// function that reads what it points at.
struct GuideRecords {
  const adx_guide* guide = nullptr;                // v1: discs and planes; iters, lambda and cap of a step
  const adx_guide_field* field = nullptr;          // v2: a cost raster
  const adx_guide_motion* motion = nullptr;        // v3: speed and acceleration limits (the row-wise kernels)
  const adx_guide_route* route = nullptr;          // v4: a route corridor
  const adx_guide_capsules* capsules = nullptr;    // v5: moving capsules
};

// An output of a launch, as the overlap refusals see it; p may be null (an optional output)
struct ByteSpan {
  const void* p;
  size_t n;
};

inline __host__ __device__ bool finite_f(float v) { return __builtin_fabsf(v) < __builtin_inff(); }      // false for inf and NaN

// u[h][d] of "warm start v1": the waypoint `shift` steps on; past the end xy go on in a straight line, the rest is held.  Shared by
// warm_init_kernel (sched.hip) and the prior of "manoeuvre commitment v1" (commit.hip), which reads a stored [H][2] plan
__device__ __forceinline__ float warm_advance(const float* p, int h, int d, int H, int D, int shift) {
#pragma clang fp contract(off)
  const int j = h + shift;
  if (j <= H - 1) return p[j * D + d];
  const float last = p[(H - 1) * D + d];
  if (d >= 2) return last;
  const float step = last - p[(H - 2) * D + d];
  const float run = (float)(j - (H - 1)) * step;
  return last + run;
}

// A [rows][horizon][dim] launch: not empty, and small enough for the kernels' int element index (and the e + total of the
// classifier-free combine)
inline int shape_check(const char* what, int rows, int horizon, int dim) {
  ADX_REQUIRE(rows >= 1 && horizon >= 1 && dim >= 1, "%s: empty shape", what);
  const int64_t per = (int64_t)horizon * dim;        // < 2^62
  const int64_t max = 0x3fffffff;
  ADX_REQUIRE(per <= max && rows * per <= max, "%s: %lld elements do not fit the kernel's 32-bit index", what,
              (long long)((uint64_t)rows * (uint64_t)per));
  return ADX_OK;
}

// One DDIM / DDPM step.  The kernel is step_kernel<ddpm, ns != null, pin != null, a guide, a field, a route or capsules>; z and ns may not
// both be given.
struct StepCall {
  bool ddpm = false;                  // which schedule: false DDIM, true DDPM
  const adx_step_coef* c = nullptr;
  const float* mo = nullptr;          // model output [batch][H][D], [2 * batch] rows when c->cfg_combine
  const float* x = nullptr;           // sample
  const float* z = nullptr;           // noise tensor, or
  const uint32_t* ns = nullptr;       // the noise stream's state: the kernel draws at (slot, row_offset)
  int32_t slot = 0;
  int64_t row_offset = 0;
  const float* tgt = nullptr;         // inpainting schedulers: known trajectory and
  const float* mask = nullptr;        // its mask
  const adx_pin* pin = nullptr;       // pinned waypoints v1
  GuideRecords g;                     // cost guidance: limits pick step_rows_kernel<ddpm, ns != null, pin != null> instead
  float* prev = nullptr;
  float* x0 = nullptr;                // optional
  int batch = 0, horizon = 0, dim = 0;
  hipStream_t stream = nullptr;
};

// One DPM-Solver++ step.  The kernel is dpm_step_kernel<pin != null, a guide, a field, a route or capsules>; without a pin the noise
// fields are not looked at.
struct DpmCall {
  const adx_dpm_coef* c = nullptr;
  const float* mo = nullptr;
  const float* x = nullptr;
  const float* px0 = nullptr;         // x0 of the previous step; null on a first-order step
  const uint32_t* ns = nullptr;       // the pin's noise (known_noise): the stream only
  int32_t slot = 0;
  int64_t row_offset = 0;
  const adx_pin* pin = nullptr;
  GuideRecords g;                     // cost guidance: limits pick dpm_step_rows_kernel<pin != null> instead
  float* prev = nullptr;
  float* x0 = nullptr;                // always written
  int batch = 0, horizon = 0, dim = 0;
  hipStream_t stream = nullptr;
};

int step_run(const StepCall& k);
int dpm_run(const DpmCall& k);
// Every refusal of "cost guidance v1" to "v5" that guided launches share, record by record in the contracts' order, each with
// `what` in front, filling the kernels' GuideArgs (field, route and capsules included) and MotionArgs.  A consumer that takes no
// limits (stop_short) passes a null `ma`: then r.motion is neither checked nor read, as if it were null.
//   the guide: dim >= 2, the counts, the arrays, scene_rows against `batch` rows; a field alone stands for a guide without discs
//     and planes.  `step`: a sampler step, which also reads iters, cap and lambda, refuses `inpaint`, and refuses a field, limits,
//     a route or capsules without a guide to read them from;
//   the field: cells, the node counts, scene_rows, the geometry, the weight;
//   the limits: the array, scene_rows, the weights, horizon <= 64;
//   the route: the arrays, the point count, scene_rows, the weight;
//   the capsules: the array, the slot count, scene_rows, the weight.
// A record's scene_rows must divide `batch` and equal that of every earlier record present (a guide without discs and planes is
// exempt), and its arrays may overlap none of the `n_outs` outputs: both refusals close the record's block.  A new term adds a
// field to GuideRecords, GuideArgs and SceneGuide, one block here and one in guide_grad, and touches no call site.
int guide_records_check(const GuideRecords& r, const char* what, bool step, bool inpaint, const ByteSpan* outs, int n_outs, int batch,
                        int horizon, int dim, GuideArgs* ga, MotionArgs* ma);
int guide_cost(const float* traj, const GuideRecords& g, float* cost, int32_t* active, int rows, int horizon, int dim, hipStream_t s);
// selection cost v1 and v2 (select.hip)
int traj_select(const adx_select_cfg* c, const float* trajs, const float* target, float* cost, int32_t* index, float* best,
                hipStream_t s);
int traj_select_guide(const adx_select_guide_cfg* c, const float* trajs, const float* target, const GuideRecords& g, float* cost,
                      int32_t* active, int32_t* index, int32_t* blocked, float* best, hipStream_t s);
// "Trajectory modes v1" (modes.hip)
int traj_modes(const adx_modes_cfg* c, const float* trajs, float* modes, int32_t* index, int32_t* mass, int32_t* assign,
               int32_t* count, float* dist2, hipStream_t s);
// "Manoeuvre commitment v1" (commit.hip)
size_t commit_state_bytes(int scenes, int horizon);
int commit_reset(void* state, int scenes, int horizon, const uint8_t* mask, hipStream_t s);
int traj_commit(const adx_commit_cfg* c, const float* trajs, const float* cost, const int32_t* selected, const int32_t* active,
                const float* motion, void* state, float* best, int32_t* index, int32_t* status, int32_t* follower, int32_t* blocked,
                float* dist2, hipStream_t s);
// "Ego frame v1" and "route planner v1" (nav.hip)
size_t nav_state_bytes(int scenes);
int nav_reset(void* state, int scenes, const uint8_t* mask, hipStream_t s);
int nav_step(const adx_nav_cfg* c, const double* route, const int32_t* cmd, const int32_t* len, const double* pose, void* state,
             float* target, int32_t* command, float* window, float* motion, int32_t* fresh, int32_t* head_out, hipStream_t s);
int world_to_ego(int kind, const double* in, const double* pose, float* out, int scenes, int n, double xy_scale, double vel_scale,
                 hipStream_t s);
int ego_to_world(const float* plans, const double* pose, double* out, int rows, int scenes, int horizon, int dim, double xy_scale,
                 hipStream_t s);
// "Vehicle v1" (vehicle.hip)
size_t vehicle_state_bytes(int scenes);
int vehicle_reset(void* state, int scenes, const double* pose, const double* speed, const uint8_t* mask, double* pose_out,
                  float* velocity_out, float* yaw_rate_out, hipStream_t s);
int vehicle_step(const adx_vehicle_cfg* c, const float* control, const int32_t* hold, void* state, double* pose, float* velocity,
                 float* yaw_rate, hipStream_t s);
// "Drive metrics v1" (drive.hip)
size_t drive_state_bytes(int scenes);
int drive_reset(void* state, int scenes, const uint8_t* mask, int32_t* done, hipStream_t s);
int drive_step(const adx_drive_cfg* c, const double* pose, const float* velocity, const float* yaw_rate, const double* route,
               const int32_t* len, const double* cum, const double* discs, const double* boxes, void* state, int32_t* done,
               hipStream_t s);
// "Signals v1" (signals.hip)
size_t signals_state_bytes(int scenes);
int signals_reset(void* state, int scenes, const uint8_t* mask, float* planes_out, int n_planes, hipStream_t s);
int signals_step(const adx_signals_cfg* c, const double* signals, const double* pose, const float* velocity, const int32_t* hold,
                 void* state, float* planes, int32_t* phase, hipStream_t s);
// "Traffic v1" (traffic.hip)
size_t traffic_state_bytes(int scenes, int n_agents);
int traffic_reset(const adx_traffic_cfg* c, const double* paths, const int32_t* plen, const double* cum, const double* heading,
                  const double* agents, const uint8_t* mask, void* state, double* boxes, int32_t* leader, hipStream_t s);
int traffic_step(const adx_traffic_cfg* c, const double* paths, const int32_t* plen, const double* cum, const double* heading,
                 const double* agents, const double* stops, const int32_t* phase, const double* pose, const float* velocity,
                 const int32_t* hold, void* state, double* boxes, int32_t* leader, hipStream_t s);
// "Camera v1" (camera.hip)
size_t camera_prims_bytes(const adx_camera_cfg* c);
void camera_default_palette(uint8_t* palette, uint8_t* shade);
int camera_render(const adx_camera_cfg* c, const double* pose, const double* boxes, const double* discs, const double* signals,
                  const int32_t* phase, const double* roads, const int32_t* road_len, const int32_t* hold, void* prims, uint8_t* frames,
                  float* image, int32_t* ids, float* depth, hipStream_t s);
// "Expert v1" (expert.hip)
int expert_plan(const adx_expert_cfg* c, const float* window, const float* velocity, const float* boxes, const float* discs,
                const float* planes, float* plan, int32_t* leader, float* info, hipStream_t s);
// "Stop-short fallback v1" (fallback.hip); g.motion is not looked at: the fallback re-times waypoints one by one
int stop_short(const float* traj, const GuideRecords& g, const float* params, int param_rows, float* out, int32_t* first,
               int32_t* status, float* stop_at, int32_t* active_after, int rows, int horizon, int dim, hipStream_t s);
// "Open-loop metrics v1" (metrics.hip)
int traj_metrics(const adx_metrics_cfg* c, const float* trajs, const float* gt, const int32_t* valid, const int32_t* index, float* ade,
                 float* fde, int32_t* best, float* rec, int32_t* flags, float* disp_sel, hipStream_t s);
size_t metrics_state_bytes();
int metrics_reset(void* state, hipStream_t s);
int metrics_accumulate(void* state, const float* rec, const int32_t* flags, const int32_t* best, const int32_t* index,
                       const float* disp_sel, const int32_t* blocked, int scenes, int horizon, hipStream_t s);
// "Capsules from boxes v1" (capsule.hip)
int capsules_from_boxes(const float* boxes, float* out, int scenes, int n_boxes, float inflate, hipStream_t s);
int field_from_occupancy(const float* occ, float* cells, int scenes, int gy, int gx, float dx, float dy, float inv_m2, int ry, int rx,
                         hipStream_t s);
int pin_apply(float* x, const adx_pin* pin, const uint32_t* ns, int64_t row_offset, int batch, int horizon, int dim, hipStream_t s);
int noise_normal(const uint32_t* state, int32_t slot, int64_t first, float* out, int64_t n, hipStream_t s);
int noise_words(const uint32_t* state, int32_t slot, int64_t first, uint32_t* out, int64_t n, hipStream_t s);
int noise_advance(uint32_t* state, hipStream_t s);
int warm_init(const float* prev, int prev_rows, const float* motion, float* out, int rows, int horizon, int dim, int shift,
              float sqrt_ab, float sqrt_1mab, const uint32_t* ns, int64_t row_offset, int zero_first, hipStream_t s);
int add_noise(const float* x, const float* n, const int64_t* t, const float* sa, const float* sb, int n_train, float* out,
              int batch, int horizon, int dim, int zero_first, hipStream_t s);
int image_normalize(const uint8_t* src, float* dst, int n, int h, int w, const float* mean, const float* stdv, hipStream_t s);

}  // namespace adx
