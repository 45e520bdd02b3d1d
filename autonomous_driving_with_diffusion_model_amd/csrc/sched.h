// Entries of sched.hip.  A scheduler step is described by ONE record with named fields and run by ONE function: the exports of
// api.cpp fill a StepCall / DpmCall and step_run / dpm_run validate it, pick the kernel instantiation and launch.
#pragma once
#include "adx_common.h"
#include "guide.h"

namespace adx {

// One DDIM / DDPM step.  The kernel is step_kernel<ddpm, ns != null, pin != null, guide != null || field != null>; z and ns may not
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
  const adx_guide* guide = nullptr;   // cost guidance v1
  const adx_guide_field* field = nullptr;      // cost guidance v2: the GUIDE kernel with a raster
  const adx_guide_motion* motion = nullptr;    // cost guidance v3: step_rows_kernel<ddpm, ns != null, pin != null> instead
  const adx_guide_route* route = nullptr;      // cost guidance v4: a route corridor in whichever kernel runs
  const adx_guide_capsules* capsules = nullptr;      // cost guidance v5: moving capsules in whichever kernel runs
  float* prev = nullptr;
  float* x0 = nullptr;                // optional
  int batch = 0, horizon = 0, dim = 0;
  hipStream_t stream = nullptr;
};

// One DPM-Solver++ step.  The kernel is dpm_step_kernel<pin != null, guide != null || field != null>; without a pin the noise
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
  const adx_guide* guide = nullptr;   // cost guidance v1
  const adx_guide_field* field = nullptr;      // cost guidance v2
  const adx_guide_motion* motion = nullptr;    // cost guidance v3: dpm_step_rows_kernel<pin != null> instead
  const adx_guide_route* route = nullptr;      // cost guidance v4
  const adx_guide_capsules* capsules = nullptr;      // cost guidance v5
  float* prev = nullptr;
  float* x0 = nullptr;                // always written
  int batch = 0, horizon = 0, dim = 0;
  hipStream_t stream = nullptr;
};

int step_run(const StepCall& k);
int dpm_run(const DpmCall& k);
// The refusals of "cost guidance v1" that every guided launch shares, filling the kernels' GuideArgs: dim >= 2, the counts, the
// arrays, scene_rows against `batch` rows, and `out` [on bytes] / `out2` [on2 bytes, may be null] against discs and planes.
// `step`: a sampler step, which also reads iters, cap and lambda and refuses `inpaint`.  `what` prefixes every text.
// `f`: the field of "cost guidance v2" or null; with a field `g` may be null (no discs, no planes) unless `step`.  The field's
// refusals follow the guide's: cells, the node counts, its scene_rows against `batch` and against the guide's, the geometry, the
// weight, and the outputs against cells.
int guide_check(const adx_guide* g, const adx_guide_field* f, const char* what, bool step, bool inpaint, const void* out, size_t on,
                const void* out2, size_t on2, int batch, int dim, GuideArgs* a);
// The refusals of "cost guidance v3" that every launch with motion limits shares, after guide_check, filling MotionArgs: the
// limits, their scene_rows against `batch` and against the guide's and the field's, the weights, horizon <= 64 and the outputs
// against the limits.  `g` and `f` are the (checked) guide and field beside it; either may be null.
int motion_check(const adx_guide_motion* m, const adx_guide* g, const adx_guide_field* f, const char* what, const void* out, size_t on,
                 const void* out2, size_t on2, int batch, int horizon, MotionArgs* a);
// The refusals of "cost guidance v4" that every launch with a route shares, after guide_check (which leaves GuideArgs without a
// route) and motion_check, filling RouteArgs: the arrays, the point count, scene_rows against `batch` and against the guide's, the
// field's and the limits', the weight and the outputs against the arrays.  `g`, `f` and `m` are the (checked) records beside it;
// each may be null.
int route_check(const adx_guide_route* r, const adx_guide* g, const adx_guide_field* f, const adx_guide_motion* m, const char* what,
                const void* out, size_t on, const void* out2, size_t on2, int batch, RouteArgs* a);
// The refusals of "cost guidance v5" that every launch with capsules shares, after guide_check (which leaves GuideArgs without
// capsules), motion_check and route_check, filling CapsuleArgs: the array, the slot count, scene_rows against `batch` and against the
// guide's, the field's, the limits' and the route's, the weight and the outputs against the array.  `g`, `f`, `m` and `r` are the
// (checked) records beside it; each may be null.
int capsule_check(const adx_guide_capsules* c, const adx_guide* g, const adx_guide_field* f, const adx_guide_motion* m,
                  const adx_guide_route* r, const char* what, const void* out, size_t on, const void* out2, size_t on2, int batch,
                  CapsuleArgs* a);
int guide_cost(const float* traj, const adx_guide* guide, const adx_guide_field* field, const adx_guide_motion* motion,
               const adx_guide_route* route, const adx_guide_capsules* capsules, float* cost, int32_t* active, int rows, int horizon,
               int dim, hipStream_t s);
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
