// Scheduler step arithmetic: one fused elementwise kernel per denoising step.
//
//   S1 GuidanceDDIMScheduler.step    scheduler/guidance_ddim_scheduler.py:60-173
//   S2 GuidanceDDPMScheduler.step    scheduler/guidance_ddpm_scheduler.py:59-178 (== stock diffusers DDPM, train.py:87)
//   S3 InpaintingDDIMScheduler.step  scheduler/inpainting_ddim_scheduler.py:10-153
//   S4 InpaintingDDPMScheduler.step  scheduler/inpainting_ddpm_scheduler.py:10-146
//   C1 classifier-free combine       interact.py:142-144
//   C2 trajs[:, 0, :3] = 0           interact.py:164, train.py:88
//   add_noise                        diffusers DDPMScheduler.add_noise, train.py:234-235
//
// The reference evaluates these as ~10 separate torch ops on [B,H,7] tensors with 0-dim CPU
// coefficients (a host sync per step).  Here the host passes the fp32-rounded scalars by value
// and the kernel repeats the reference's elementwise operations in the same order with
// contraction disabled, so results are bit-identical to the torch CPU path.
//
//
// The step's Gaussian term comes from one of two sources, chosen at compile time: a noise TENSOR the caller drew (the
// reference's path: torch.randn, or an injected variance_noise), or the counter-based noise stream of csrc/noise.h, evaluated
// in the kernel where the tensor element would be read (adx_*_step_rng: no launch, no allocation, no [B,H,D] round trip, and a
// captured graph draws fresh noise on every replay because the stream's state is read through a pointer).
//
// "Pinned waypoints v1" (include/adx.h) is a compile-time variant of both step kernels (PIN): the finished prev_sample is blended
// with the caller's known trajectory under a mask before zero_first has the last word.  The unpinned instantiations do not read
// the pin fields, which sit behind every field they do read: their code is what it was.
//
// "Cost guidance v1" (include/adx.h) is one more compile-time variant (GUIDE): after the step's own clip, an xy thread recomputes
// its partner element's x0, walks the waypoint down the gradient of the scene's disc and half-plane cost and, where its own element
// moved, runs the rest of the step from the moved x0.  The gradient is one __device__ helper (guide.h), shared with guide_cost_kernel.  The
// unguided instantiations do not read the guide fields, which sit behind the pin's: their code is what it was.
// "Cost guidance v2" adds a cost raster to that helper and no kernel variant: the GUIDE instantiations branch on the record's
// `cells != nullptr`, which is the same in every thread of a launch.
// "Cost guidance v3" (motion limits) couples neighbouring waypoints and gets kernels of its own, step_rows_kernel and
// dpm_step_rows_kernel: a wave per row, the iterate exchanged by shuffles.  The body of one element's step is text both kernel
// shapes include (sched_step_body.h, sched_dpm_body.h), so the element-wise instantiations compile from the tokens they had.
//
// Host side (sched.h): every step export fills one record, StepCall or DpmCall, and one function, step_run or dpm_run, checks it
// and picks the kernel instantiation from what the record holds (schedule, noise state or not, pin or not, guide or not).  Every refusal of a
// step lives in those two functions and the helpers they share with pin_apply, warm_init and add_noise: shape_check (non-empty,
// fits the kernels' 32-bit index), noise_rows (the launch's rows inside the stream), pin_check (what is pin-specific) and
// guide_records_check (what the guide records of a launch ask, all five in one pass; guide_cost, select.hip and fallback.hip share it).
// Device side: the arithmetic two kernels share is written once, in __device__ helpers that keep the reference's operation order.
#include "sched.h"
#include "noise.h"

namespace adx {

// Pinned waypoints v1: known / mask [known_rows][H][D], `span` = known_rows * H * D: element e of a launch reads e % span, i.e. row
// r reads known row r % known_rows
struct PinArgs {
  const float* known;
  const float* mask;
  int span;
  float c_known, c_known_noise;
  int known_noise;
};

// prev = mask * kp + (1 - mask) * prev at element i of known / mask, kp = c_known * known + (known_noise ? c_known_noise * z : 0):
// the RePaint blend of the inpainting steps and of a pin, every product and sum rounded on its own
__device__ __forceinline__ float repaint_blend(const float* known, const float* mask, int i, float c_known, float c_known_noise,
                                               int known_noise, float z, float prev) {
#pragma clang fp contract(off)
  const float k0 = c_known * known[i];
  const float k1 = known_noise ? c_known_noise * z : 0.f;
  const float kp = k0 + k1;
  const float mk = mask[i];
  const float u = mk * kp, v = (1.0f - mk) * prev;
  return u + v;
}

__device__ __forceinline__ float pin_blend(const PinArgs& p, int e, float z, float prev) {
  return repaint_blend(p.known, p.mask, e % p.span, p.c_known, p.c_known_noise, p.known_noise, z, prev);
}

// C1: uncond + free_scale * (cond - uncond) of a [2 * rows] model output, rows [0, rows) cond; else the model output itself
__device__ __forceinline__ float cfg_model_output(const float* mo, int e, int total, int cfg_combine, float free_scale) {
#pragma clang fp contract(off)
  if (cfg_combine) {
    const float cnd = mo[e], unc = mo[e + total];
    const float d = cnd - unc;
    const float sd = free_scale * d;
    return unc + sd;
  }
  return mo[e];
}

// pred_original_sample before the clamp, from the model output m at signal level sa and noise level sb
__device__ __forceinline__ float x0_from(int prediction_type, float sa, float sb, float xs, float m) {
#pragma clang fp contract(off)
  if (prediction_type == ADX_PRED_EPSILON) {
    const float p = sb * m;
    return (xs - p) / sa;
  }
  if (prediction_type == ADX_PRED_SAMPLE) return m;
  const float p = sa * xs, q = sb * m;
  return p - q;
}

// C2: element e of a [rows][horizon][dim] tensor lies in [:, 0, :3]
__device__ __forceinline__ bool first_pose(int e, int horizon, int dim) {
  const int d = e % dim;
  const int h = (e / dim) % horizon;
  return h == 0 && d < 3;
}

struct StepArgs {
  adx_step_coef c;
  const float* mo;
  const float* x;
  const float* z;
  const float* tgt;
  const float* mask;
  float* prev;
  float* x0;
  int total, horizon, dim;
  // noise stream (RNG kernels only): state words, slot = the integer timestep, first logical element of this launch's rows
  const uint32_t* ns;
  uint32_t slot;
  uint64_t base;
  // pinned waypoints v1 (PIN kernels only)
  PinArgs pin;
  // cost guidance v1 (GUIDE kernels only)
  GuideArgs guide;
};

__device__ __forceinline__ float clamp_nan(float v, float lo, float hi) {
  // torch.clamp propagates NaN
  return v < lo ? lo : (v > hi ? hi : v);
}

// The guide of one step at element e, whose clipped pred_original_sample is x0.  An xy element (d < 2; the host checked dim >= 2)
// recomputes its partner's x0 through the step's own helpers, repeats the waypoint's iterations and, if its own component moved,
// leaves the guided value in x0 and returns true.  (pt, sa, sb): the operands of x0_from at this step.
__device__ __forceinline__ bool guide_x0(const GuideArgs& g, const float* mo, const float* x, int e, int total, int horizon, int dim,
                                         int pt, float sa, float sb, int clip, float clip_range, int cfg_combine, float free_scale,
                                         float& x0) {
#pragma clang fp contract(off)
  const int d = e % dim;
  if (d >= 2) return false;
  const int w = e / dim;
  const int h = w % horizon, row = w / horizon, scene_index = row % g.scene_rows;      // here, ahead of the partner's loads
  const int ep = d == 0 ? e + 1 : e - 1;                 // the waypoint's other xy element
  float xp = x0_from(pt, sa, sb, x[ep], cfg_model_output(mo, ep, total, cfg_combine, free_scale));
  if (clip) xp = clamp_nan(xp, -clip_range, clip_range);
  float px = d == 0 ? x0 : xp, py = d == 0 ? xp : x0;
  const SceneGuide scene = scene_guide(g, row, scene_index);
  const float hf = (float)h;
  bool moved = false;
  for (int it = 0; it < g.iters; ++it) {
    float J, gx, gy;
    int active;
    guide_grad(scene, hf, px, py, J, gx, gy, active);
    const float lx = g.lambda * gx, ly = g.lambda * gy;
    const float sx = clamp_nan(lx, -g.cap, g.cap), sy = clamp_nan(ly, -g.cap, g.cap);
    moved = moved || (d == 0 ? sx : sy) != 0.f;
    px = px - sx;
    py = py - sy;
    if (clip) {
      px = clamp_nan(px, -clip_range, clip_range);
      py = clamp_nan(py, -clip_range, clip_range);
    }
  }
  if (moved) x0 = d == 0 ? px : py;
  return moved;
}

template <bool DDPM, bool RNG, bool PIN, bool GUIDE>
__global__ void __launch_bounds__(256) step_kernel(const StepArgs a) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.total) return;
  constexpr bool ROWS = false, row_moved = false;
  constexpr float row_x0 = 0.f;
#include "sched_step_body.h"
}

// "Cost guidance v3" (include/adx.h): the motion terms couple a waypoint to its neighbours, so the iterations cannot be local to
// an element.  The row-wise kernels give a row to a wave: lane = waypoint, four rows per workgroup, nothing shared between the
// waves (no LDS, no atomics, no barrier).  A lane owns both xy elements of its waypoint, so there is no partner recomputation; the
// iterate travels to the neighbours through wave shuffles after every move (Jacobi), and all 64 lanes stay alive through them:
// lanes h >= H hold zeros, take no step and touch no memory.  Every trip count is the launch's.
constexpr int kRowWaves = 4;

// The clipped pred_original_sample of one element: where a row's iterations start
__device__ __forceinline__ float x0_clipped(int pt, float sa, float sb, float xs, float m, int clip, float clip_range) {
  const float x0 = x0_from(pt, sa, sb, xs, m);
  return clip ? clamp_nan(x0, -clip_range, clip_range) : x0;
}

// The iterations of one row: (px, py) is the lane's clipped x0 on entry and the iterate on exit, (mx, my) whether a component
// moved.  `live`: lane < H.
__device__ __forceinline__ void guide_rows(const GuideArgs& g, const MotionArgs& mo, int row, int lane, int H, bool live, int clip,
                                           float clip_range, float& px, float& py, bool& mx, bool& my) {
#pragma clang fp contract(off)
  const SceneGuide scene = scene_guide(g, row);
  float S2, A2;
  motion_limits(mo, row, S2, A2);
  const float hf = (float)lane;
  mx = false; my = false;
  for (int it = 0; it < g.iters; ++it) {
    float nx[5], ny[5];
    nx[0] = __shfl_up(px, 2, kWave); ny[0] = __shfl_up(py, 2, kWave);
    nx[1] = __shfl_up(px, 1, kWave); ny[1] = __shfl_up(py, 1, kWave);
    nx[2] = px; ny[2] = py;
    nx[3] = __shfl_down(px, 1, kWave); ny[3] = __shfl_down(py, 1, kWave);
    nx[4] = __shfl_down(px, 2, kWave); ny[4] = __shfl_down(py, 2, kWave);
    if (live) {
      float J, gx, gy;
      int active;
      guide_grad(scene, hf, px, py, J, gx, gy, active);
      motion_grad(nx, ny, lane, H, S2, A2, mo.w_speed, mo.w_accel, J, gx, gy, active);
      const float lx = g.lambda * gx, ly = g.lambda * gy;
      const float sx = clamp_nan(lx, -g.cap, g.cap), sy = clamp_nan(ly, -g.cap, g.cap);
      mx = mx || sx != 0.f;
      my = my || sy != 0.f;
      px = px - sx;
      py = py - sy;
      if (clip) {
        px = clamp_nan(px, -clip_range, clip_range);
        py = clamp_nan(py, -clip_range, clip_range);
      }
    }
  }
}

struct StepRowsArgs {
  StepArgs s;
  MotionArgs motion;      // cost guidance v3
};

template <bool DDPM, bool RNG, bool PIN>
__global__ void __launch_bounds__(kRowWaves * kWave) step_rows_kernel(const StepRowsArgs k) {
#pragma clang fp contract(off)
  const StepArgs& a = k.s;
  const adx_step_coef& c = a.c;
  const int lane = threadIdx.x & (kWave - 1);
  const int H = a.horizon, D = a.dim;
  const int row = blockIdx.x * kRowWaves + (threadIdx.x >> 6);
  if (row >= a.total / (H * D)) return;              // whole waves leave: the shuffles always see all 64 lanes
  const bool live = lane < H;
  const int e0 = (row * H + lane) * D;               // the waypoint's x element; live lanes only read or write there
  float px = 0.f, py = 0.f;
  if (live) {
    px = x0_clipped(c.prediction_type, c.sqrt_alpha_t, c.sqrt_beta_t, a.x[e0], cfg_model_output(a.mo, e0, a.total, c.cfg_combine, c.free_scale),
                    c.clip, c.clip_range);
    py = x0_clipped(c.prediction_type, c.sqrt_alpha_t, c.sqrt_beta_t, a.x[e0 + 1],
                    cfg_model_output(a.mo, e0 + 1, a.total, c.cfg_combine, c.free_scale), c.clip, c.clip_range);
  }
  bool mx, my;
  guide_rows(a.guide, k.motion, row, lane, H, live, c.clip, c.clip_range, px, py, mx, my);
  if (!live) return;                                  // no shuffle below this line
  constexpr bool GUIDE = false, ROWS = true;
  for (int d = 0; d < D; ++d) {                       // the waypoint's D elements, each through the element kernel's own body
    const int e = e0 + d;
    const float row_x0 = d == 0 ? px : py;
    const bool row_moved = d == 0 ? mx : (d == 1 ? my : false);
#include "sched_step_body.h"
  }
}

// e >> 2 is the stream's 32-bit counter word: logical elements live in [0, 2^34)
static const int64_t kNoiseElems = (int64_t)1 << 34;

// Rows [row_offset, row_offset + rows) of `per` >= 1 elements each lie inside the noise stream; *base = their first logical element
static int noise_rows(const char* what, int64_t row_offset, int rows, int64_t per, uint64_t* base) {
  ADX_REQUIRE(row_offset >= 0, "%s: negative row_offset %lld", what, (long long)row_offset);
  ADX_REQUIRE(row_offset <= kNoiseElems && (row_offset + rows) <= kNoiseElems / per,
              "%s: rows [%lld, %lld) of %lld elements leave the noise stream's 2^34 elements", what, (long long)row_offset,
              (long long)row_offset + rows, (long long)per);
  *base = (uint64_t)row_offset * (uint64_t)per;
  return ADX_OK;
}

// the refusals of "pinned waypoints v1" that every pinned launch shares, after shape_check; `out2` may be null
static int pin_check(const adx_pin* pin, const char* what, bool has_noise, const float* out, const float* out2, int batch, int horizon,
                     int dim, PinArgs* p) {
  ADX_REQUIRE(pin->known != nullptr && pin->mask != nullptr, "%s: null known or mask", what);
  ADX_REQUIRE(pin->known_rows >= 1 && batch % pin->known_rows == 0, "%s: batch %d must be a positive multiple of known_rows %d", what,
              batch, pin->known_rows);
  ADX_REQUIRE(!pin->known_noise || has_noise, "%s: known_noise is set and there is no noise tensor and no noise state", what);
  const int64_t per = (int64_t)horizon * dim;
  const size_t kn = (size_t)pin->known_rows * per * sizeof(float), on = (size_t)batch * per * sizeof(float);
  ADX_REQUIRE(!byte_ranges_overlap(out, on, pin->known, kn) && !byte_ranges_overlap(out, on, pin->mask, kn) &&
              (out2 == nullptr || (!byte_ranges_overlap(out2, on, pin->known, kn) && !byte_ranges_overlap(out2, on, pin->mask, kn))),
              "%s: an output overlaps known or mask", what);
  p->known = pin->known; p->mask = pin->mask; p->span = (int)(pin->known_rows * per);
  p->c_known = pin->c_known; p->c_known_noise = pin->c_known_noise; p->known_noise = pin->known_noise != 0;
  return ADX_OK;
}

static const FieldArgs kNoField = {nullptr, 1, 2, 2, 0.f, 0.f, 0.f, 0.f, 0.f};
static const RouteArgs kNoRoute = {nullptr, nullptr, 1, 2, 0.f};
static const CapsuleArgs kNoCapsule = {nullptr, 1, 1, 0.f};
static const GuideArgs kNoGuide = {nullptr, nullptr, 1, 0, 0, 0, 0.f, 0.f, kNoField, kNoRoute, kNoCapsule};

// One record's scene count as the agreement refusals name it: "<holds> %d scenes, <beside> %d"
struct SceneCount {
  const char* holds;      // as the record that disagrees
  const char* beside;     // as the earlier record it disagrees with
  bool binds;             // present, and not a guide without discs and planes
  int scenes;
};

// record `i` of `t` against every earlier record that binds
static int scenes_agree(const char* what, const SceneCount* t, int i) {
  for (int j = 0; j < i; ++j)
    ADX_REQUIRE(!t[j].binds || t[j].scenes == t[i].scenes, "%s: %s %d scenes, %s %d", what, t[i].holds, t[i].scenes, t[j].beside,
                t[j].scenes);
  return ADX_OK;
}

// some output shares a byte with [q, q + qn)
static bool outputs_overlap(const ByteSpan* outs, int n_outs, const void* q, size_t qn) {
  for (int i = 0; i < n_outs; ++i)
    if (outs[i].p != nullptr && byte_ranges_overlap(outs[i].p, outs[i].n, q, qn)) return true;
  return false;
}

// every refusal the guide records of a launch share (sched.h)
int guide_records_check(const GuideRecords& r, const char* what, bool step, bool inpaint, const ByteSpan* outs, int n_outs, int batch,
                        int horizon, int dim, GuideArgs* ga, MotionArgs* ma) {
  static const adx_guide bare = {nullptr, nullptr, 1, 0, 0, 1, 0.f, 0.f};      // a field without a guide: no discs, no planes
  const adx_guide* g = r.guide;
  const adx_guide_field* const f = r.field;
  const adx_guide_motion* const m = ma != nullptr ? r.motion : nullptr;      // no MotionArgs to fill: the consumer takes no limits
  const adx_guide_route* const rt = r.route;
  const adx_guide_capsules* const c = r.capsules;
  if (step) {
    ADX_REQUIRE(rt == nullptr || g != nullptr, "%s: a route without a guide: a step reads iters, lambda and cap from the guide", what);
    ADX_REQUIRE(c == nullptr || g != nullptr, "%s: capsules without a guide: a step reads iters, lambda and cap from the guide", what);
    ADX_REQUIRE(m == nullptr || g != nullptr, "%s: motion limits without a guide: a step reads iters, lambda and cap from the guide", what);
  }
  if (g == nullptr) {
    ADX_REQUIRE(f != nullptr, "%s: null guide", what);
    ADX_REQUIRE(!step, "%s: a field without a guide: a step reads iters, lambda and cap from the guide", what);
    g = &bare;
  }
  const SceneCount held[5] = {
      {nullptr, "the guide's discs and planes", g->n_discs != 0 || g->n_planes != 0, g->scene_rows},
      {"the field holds", "the field", f != nullptr, f != nullptr ? f->scene_rows : 0},
      {"the limits hold", "the motion limits", m != nullptr, m != nullptr ? m->scene_rows : 0},
      {"the route holds", "the route", rt != nullptr, rt != nullptr ? rt->scene_rows : 0},
      {"the capsules hold", nullptr, c != nullptr, c != nullptr ? c->scene_rows : 0}};
  int rc;

  // cost guidance v1: discs and planes
  ADX_REQUIRE(dim >= 2, "%s: cost guidance moves (x, y), dim is %d", what, dim);
  ADX_REQUIRE(g->n_discs >= 0 && g->n_discs <= ADX_GUIDE_MAX_DISCS, "%s: n_discs %d outside 0..%d", what, g->n_discs,
              ADX_GUIDE_MAX_DISCS);
  ADX_REQUIRE(g->n_planes >= 0 && g->n_planes <= ADX_GUIDE_MAX_PLANES, "%s: n_planes %d outside 0..%d", what, g->n_planes,
              ADX_GUIDE_MAX_PLANES);
  ADX_REQUIRE(g->discs != nullptr || g->n_discs == 0, "%s: null discs with n_discs %d", what, g->n_discs);
  ADX_REQUIRE(g->planes != nullptr || g->n_planes == 0, "%s: null planes with n_planes %d", what, g->n_planes);
  ADX_REQUIRE(g->scene_rows >= 1 && batch % g->scene_rows == 0, "%s: batch %d must be a positive multiple of scene_rows %d", what,
              batch, g->scene_rows);
  if (step) {
    ADX_REQUIRE(g->iters >= 1 && g->iters <= ADX_GUIDE_MAX_ITERS, "%s: guide iters %d outside 1..%d", what, g->iters,
                ADX_GUIDE_MAX_ITERS);
    ADX_REQUIRE(g->cap >= 0.f, "%s: guide cap %g is negative or NaN", what, (double)g->cap);
    ADX_REQUIRE(g->lambda == g->lambda, "%s: guide lambda is NaN", what);
    ADX_REQUIRE(!inpaint, "%s: c->inpaint (the inpainting schedulers' blend) and a guide do not compose", what);
  }
  ADX_REQUIRE(!outputs_overlap(outs, n_outs, g->discs, (size_t)g->scene_rows * g->n_discs * 5 * sizeof(float)) &&
                  !outputs_overlap(outs, n_outs, g->planes, (size_t)g->scene_rows * g->n_planes * 3 * sizeof(float)),
              "%s: an output overlaps discs or planes", what);
  *ga = kNoGuide;
  ga->discs = g->discs; ga->planes = g->planes; ga->scene_rows = g->scene_rows; ga->M = g->n_discs; ga->P = g->n_planes;
  ga->iters = g->iters; ga->lambda = g->lambda; ga->cap = g->cap;
  if (ma != nullptr) *ma = MotionArgs{nullptr, 1, 0.f, 0.f};

  if (f != nullptr) {      // cost guidance v2: the field
    ADX_REQUIRE(f->cells != nullptr, "%s: null field cells", what);
    ADX_REQUIRE(f->gx >= ADX_FIELD_MIN_NODES && f->gx <= ADX_FIELD_MAX_NODES && f->gy >= ADX_FIELD_MIN_NODES &&
                f->gy <= ADX_FIELD_MAX_NODES, "%s: field of %d x %d nodes (gy x gx), supported %d..%d each", what, f->gy, f->gx,
                ADX_FIELD_MIN_NODES, ADX_FIELD_MAX_NODES);
    ADX_REQUIRE(f->scene_rows >= 1 && batch % f->scene_rows == 0, "%s: batch %d must be a positive multiple of the field's scene_rows %d",
                what, batch, f->scene_rows);
    if ((rc = scenes_agree(what, held, 1)) != ADX_OK) return rc;
    ADX_REQUIRE(finite_f(f->inv_dx) && f->inv_dx > 0.f && finite_f(f->inv_dy) && f->inv_dy > 0.f,
                "%s: field inv_dx %g and inv_dy %g must be finite and > 0", what, (double)f->inv_dx, (double)f->inv_dy);
    ADX_REQUIRE(f->weight >= 0.f, "%s: field weight %g is negative or NaN", what, (double)f->weight);
    ADX_REQUIRE(finite_f(f->x_min) && finite_f(f->y_min), "%s: field origin (%g, %g) is not finite", what, (double)f->x_min,
                (double)f->y_min);
    ADX_REQUIRE(!outputs_overlap(outs, n_outs, f->cells, (size_t)f->scene_rows * f->gy * f->gx * sizeof(float)),
                "%s: an output overlaps the field's cells", what);
    ga->field = FieldArgs{f->cells, f->scene_rows, f->gx, f->gy, f->x_min, f->y_min, f->inv_dx, f->inv_dy, f->weight};
  }

  if (m != nullptr) {      // cost guidance v3: the motion limits
    ADX_REQUIRE(m->limits != nullptr, "%s: null motion limits", what);
    ADX_REQUIRE(m->scene_rows >= 1 && batch % m->scene_rows == 0, "%s: batch %d must be a positive multiple of the limits' scene_rows %d",
                what, batch, m->scene_rows);
    if ((rc = scenes_agree(what, held, 2)) != ADX_OK) return rc;
    ADX_REQUIRE(m->w_speed >= 0.f, "%s: motion w_speed %g is negative or NaN", what, (double)m->w_speed);
    ADX_REQUIRE(m->w_accel >= 0.f, "%s: motion w_accel %g is negative or NaN", what, (double)m->w_accel);
    ADX_REQUIRE(horizon <= kWave, "%s: motion limits give a row to a wave: horizon %d, supported 1..%d", what, horizon, kWave);
    ADX_REQUIRE(!outputs_overlap(outs, n_outs, m->limits, (size_t)m->scene_rows * 2 * sizeof(float)),
                "%s: an output overlaps the motion limits", what);
    *ma = MotionArgs{m->limits, m->scene_rows, m->w_speed, m->w_accel};
  }

  if (rt != nullptr) {      // cost guidance v4: the route
    ADX_REQUIRE(rt->points != nullptr, "%s: null route points", what);
    ADX_REQUIRE(rt->half_width != nullptr, "%s: null route half_width", what);
    ADX_REQUIRE(rt->n_points >= ADX_ROUTE_MIN_POINTS && rt->n_points <= ADX_ROUTE_MAX_POINTS, "%s: route of %d points, supported %d..%d",
                what, rt->n_points, ADX_ROUTE_MIN_POINTS, ADX_ROUTE_MAX_POINTS);
    ADX_REQUIRE(rt->scene_rows >= 1 && batch % rt->scene_rows == 0, "%s: batch %d must be a positive multiple of the route's scene_rows %d",
                what, batch, rt->scene_rows);
    if ((rc = scenes_agree(what, held, 3)) != ADX_OK) return rc;
    ADX_REQUIRE(rt->weight >= 0.f, "%s: route weight %g is negative or NaN", what, (double)rt->weight);
    ADX_REQUIRE(!outputs_overlap(outs, n_outs, rt->points, (size_t)rt->scene_rows * rt->n_points * 2 * sizeof(float)) &&
                    !outputs_overlap(outs, n_outs, rt->half_width, (size_t)rt->scene_rows * sizeof(float)),
                "%s: an output overlaps the route's points or half_width", what);
    ga->route = RouteArgs{rt->points, rt->half_width, rt->scene_rows, rt->n_points, rt->weight};
  }

  if (c != nullptr) {      // cost guidance v5: the capsules
    ADX_REQUIRE(c->capsules != nullptr, "%s: null capsules", what);
    ADX_REQUIRE(c->n_capsules >= 1 && c->n_capsules <= ADX_CAPSULE_MAX, "%s: n_capsules %d outside 1..%d", what, c->n_capsules,
                ADX_CAPSULE_MAX);
    ADX_REQUIRE(c->scene_rows >= 1 && batch % c->scene_rows == 0, "%s: batch %d must be a positive multiple of the capsules' scene_rows %d",
                what, batch, c->scene_rows);
    if ((rc = scenes_agree(what, held, 4)) != ADX_OK) return rc;
    ADX_REQUIRE(c->weight >= 0.f, "%s: capsule weight %g is negative or NaN", what, (double)c->weight);
    ADX_REQUIRE(!outputs_overlap(outs, n_outs, c->capsules, (size_t)c->scene_rows * c->n_capsules * 7 * sizeof(float)),
                "%s: an output overlaps the capsules", what);
    ga->capsule = CapsuleArgs{c->capsules, c->scene_rows, c->n_capsules, c->weight};
  }
  return ADX_OK;
}

int step_run(const StepCall& k) {
  using Kernel = void (*)(const StepArgs);
#define ADX_STEP_KERNELS(ddpm, rng) {{step_kernel<ddpm, rng, false, false>, step_kernel<ddpm, rng, false, true>}, \
                                     {step_kernel<ddpm, rng, true, false>, step_kernel<ddpm, rng, true, true>}}
  static const Kernel kernels[2][2][2][2] = {      // [ddpm][noise stream][pin][guide]
      {ADX_STEP_KERNELS(false, false), ADX_STEP_KERNELS(false, true)}, {ADX_STEP_KERNELS(true, false), ADX_STEP_KERNELS(true, true)}};
#undef ADX_STEP_KERNELS
  const char* const what = "scheduler step";
  const adx_step_coef* c = k.c;
  const bool rng = k.ns != nullptr, pinned = k.pin != nullptr;
  const bool guided = k.g.guide != nullptr || k.g.field != nullptr || k.g.route != nullptr || k.g.capsules != nullptr;
  ADX_REQUIRE(k.z == nullptr || !rng, "scheduler step: a noise tensor and a noise state are both given");
  ADX_REQUIRE(c && k.mo && k.x && k.prev, "scheduler step: null tensor");
  int rc = shape_check(what, k.batch, k.horizon, k.dim);
  if (rc != ADX_OK) return rc;
  ADX_REQUIRE(c->prediction_type >= 0 && c->prediction_type <= 2,
              "prediction_type given as %d must be one of `epsilon`, `sample`, or `v_prediction`", c->prediction_type);
  StepArgs a;
  a.ns = nullptr; a.slot = 0; a.base = 0;
  a.pin = PinArgs{nullptr, nullptr, 1, 0.f, 0.f, 0};
  if (pinned) {
    ADX_REQUIRE(!c->inpaint, "scheduler step: c->inpaint (the inpainting schedulers' blend) and a pin are two blends of one step");
    rc = pin_check(k.pin, what, rng || k.z != nullptr, k.prev, k.x0, k.batch, k.horizon, k.dim, &a.pin);
    if (rc != ADX_OK) return rc;
  }
  a.guide = kNoGuide;
  StepRowsArgs ra;
  if (guided || k.g.motion != nullptr) {      // cost guidance v3 (limits): the row-wise kernel; v4 (a route), v5 (capsules): in whichever runs
    const size_t on = (size_t)k.batch * k.horizon * k.dim * sizeof(float);
    const ByteSpan outs[2] = {{k.prev, on}, {k.x0, on}};
    rc = guide_records_check(k.g, what, true, c->inpaint != 0, outs, 2, k.batch, k.horizon, k.dim, &a.guide, &ra.motion);
    if (rc != ADX_OK) return rc;
  }
  if (rng) {
    rc = noise_rows(what, k.row_offset, k.batch, (int64_t)k.horizon * k.dim, &a.base);
    if (rc != ADX_OK) return rc;
    a.ns = k.ns; a.slot = (uint32_t)k.slot;
  } else {
    ADX_REQUIRE(!(c->add_noise || (c->inpaint && c->known_noise && k.tgt && k.mask)) || k.z != nullptr,
                "scheduler step: noise tensor required");
  }
  a.c = *c;
  a.mo = k.mo; a.x = k.x; a.z = k.z; a.tgt = k.tgt; a.mask = k.mask; a.prev = k.prev; a.x0 = k.x0;
  a.total = k.batch * k.horizon * k.dim; a.horizon = k.horizon; a.dim = k.dim;
  if (k.g.motion != nullptr) {
    using RowsKernel = void (*)(const StepRowsArgs);
#define ADX_ROWS_KERNELS(ddpm) {{step_rows_kernel<ddpm, false, false>, step_rows_kernel<ddpm, false, true>}, \
                                {step_rows_kernel<ddpm, true, false>, step_rows_kernel<ddpm, true, true>}}
    static const RowsKernel rows_kernels[2][2][2] = {ADX_ROWS_KERNELS(false), ADX_ROWS_KERNELS(true)};      // [ddpm][noise stream][pin]
#undef ADX_ROWS_KERNELS
    ra.s = a;
    rows_kernels[k.ddpm][rng][pinned]<<<dim3(ceil_div(k.batch, kRowWaves)), dim3(kRowWaves * kWave), 0, k.stream>>>(ra);
    ADX_LAUNCH_CHECK();
    return ADX_OK;
  }
  kernels[k.ddpm][rng][pinned][guided]<<<dim3(ceil_div(a.total, 256)), dim3(256), 0, k.stream>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

// DPM-Solver++ multistep step (order 1 and the order-2 midpoint rule; diffusers 0.28.0 DPMSolverMultistepScheduler,
// algorithm_type = "dpmsolver++", restated in scheduler/dpm.py).  The same shape as step_kernel: one thread per element, the
// host's fp32 scalars by value, every product rounded on its own and evaluated left to right.  The one thing the DDIM step
// does not have is HISTORY: the second-order term reads the x0 the previous step wrote, so x0 is always written.
struct DpmArgs {
  adx_dpm_coef c;
  const float* mo;
  const float* x;
  const float* px0;     // x0 of the previous step; null on a first-order step
  float* prev;
  float* x0;
  int total, horizon, dim;
  // pinned waypoints v1 (the PIN kernel only): the blend and, for its noise, the stream as in StepArgs
  PinArgs pin;
  const uint32_t* ns;
  uint32_t slot;
  uint64_t base;
  // cost guidance v1 (the GUIDE kernels only)
  GuideArgs guide;
};

template <bool PIN, bool GUIDE>
__global__ void __launch_bounds__(256) dpm_step_kernel(const DpmArgs a) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.total) return;
  constexpr bool ROWS = false, row_moved = false;
  constexpr float row_x0 = 0.f;
#include "sched_dpm_body.h"
}

struct DpmRowsArgs {
  DpmArgs s;
  MotionArgs motion;      // cost guidance v3
};

// step_rows_kernel's shape around the solver's arithmetic
template <bool PIN>
__global__ void __launch_bounds__(kRowWaves * kWave) dpm_step_rows_kernel(const DpmRowsArgs k) {
#pragma clang fp contract(off)
  const DpmArgs& a = k.s;
  const adx_dpm_coef& c = a.c;
  const int lane = threadIdx.x & (kWave - 1);
  const int H = a.horizon, D = a.dim;
  const int row = blockIdx.x * kRowWaves + (threadIdx.x >> 6);
  if (row >= a.total / (H * D)) return;              // whole waves leave: the shuffles always see all 64 lanes
  const bool live = lane < H;
  const int e0 = (row * H + lane) * D;
  float px = 0.f, py = 0.f;
  if (live) {
    px = x0_clipped(c.prediction_type, c.alpha_s, c.sigma_s, a.x[e0], cfg_model_output(a.mo, e0, a.total, c.cfg_combine, c.free_scale), c.clip,
                    c.clip_range);
    py = x0_clipped(c.prediction_type, c.alpha_s, c.sigma_s, a.x[e0 + 1], cfg_model_output(a.mo, e0 + 1, a.total, c.cfg_combine, c.free_scale),
                    c.clip, c.clip_range);
  }
  bool mx, my;
  guide_rows(a.guide, k.motion, row, lane, H, live, c.clip, c.clip_range, px, py, mx, my);
  if (!live) return;                                  // no shuffle below this line
  constexpr bool GUIDE = false, ROWS = true;
  for (int d = 0; d < D; ++d) {                       // the waypoint's D elements, each through the element kernel's own body
    const int e = e0 + d;
    const float row_x0 = d == 0 ? px : py;
    const bool row_moved = d == 0 ? mx : (d == 1 ? my : false);
#include "sched_dpm_body.h"
  }
}

// a NULL pin is adx_dpm_step: the solver itself draws nothing, the noise fields are then not looked at
int dpm_run(const DpmCall& k) {
  using Kernel = void (*)(const DpmArgs);
  static const Kernel kernels[2][2] = {{dpm_step_kernel<false, false>, dpm_step_kernel<false, true>},      // [pin][guide]
                                       {dpm_step_kernel<true, false>, dpm_step_kernel<true, true>}};
  const char* const what = "dpm step";
  const adx_dpm_coef* c = k.c;
  ADX_REQUIRE(c && k.mo && k.x && k.prev && k.x0, "dpm step: null tensor");
  int rc = shape_check(what, k.batch, k.horizon, k.dim);
  if (rc != ADX_OK) return rc;
  ADX_REQUIRE(c->prediction_type >= 0 && c->prediction_type <= 2,
              "prediction_type given as %d must be one of `epsilon`, `sample`, or `v_prediction`", c->prediction_type);
  ADX_REQUIRE(!c->second_order || k.px0 != nullptr, "dpm step: a second-order step needs the previous step's x0");
  ADX_REQUIRE(k.px0 != k.prev && k.px0 != k.x0 && k.x != k.prev && k.x != k.x0 && k.mo != k.prev && k.mo != k.x0 && k.prev != k.x0,
              "dpm step: outputs alias an input or each other");
  DpmArgs a;
  a.pin = PinArgs{nullptr, nullptr, 1, 0.f, 0.f, 0};
  a.ns = nullptr; a.slot = 0; a.base = 0;
  if (k.pin != nullptr) {
    rc = pin_check(k.pin, what, k.ns != nullptr, k.prev, k.x0, k.batch, k.horizon, k.dim, &a.pin);
    if (rc != ADX_OK) return rc;
    if (k.ns != nullptr) {
      rc = noise_rows(what, k.row_offset, k.batch, (int64_t)k.horizon * k.dim, &a.base);
      if (rc != ADX_OK) return rc;
      a.ns = k.ns; a.slot = (uint32_t)k.slot;
    }
  }
  a.guide = kNoGuide;
  const bool guided = k.g.guide != nullptr || k.g.field != nullptr || k.g.route != nullptr || k.g.capsules != nullptr;
  DpmRowsArgs ra;
  if (guided || k.g.motion != nullptr) {      // cost guidance v3 (limits): the row-wise kernel; v4 (a route), v5 (capsules): in whichever runs
    const size_t on = (size_t)k.batch * k.horizon * k.dim * sizeof(float);
    const ByteSpan outs[2] = {{k.prev, on}, {k.x0, on}};
    rc = guide_records_check(k.g, what, true, false, outs, 2, k.batch, k.horizon, k.dim, &a.guide, &ra.motion);
    if (rc != ADX_OK) return rc;
  }
  a.c = *c;
  a.mo = k.mo; a.x = k.x; a.px0 = k.px0; a.prev = k.prev; a.x0 = k.x0;
  a.total = k.batch * k.horizon * k.dim; a.horizon = k.horizon; a.dim = k.dim;
  if (k.g.motion != nullptr) {
    ra.s = a;
    if (k.pin != nullptr) dpm_step_rows_kernel<true><<<dim3(ceil_div(k.batch, kRowWaves)), dim3(kRowWaves * kWave), 0, k.stream>>>(ra);
    else dpm_step_rows_kernel<false><<<dim3(ceil_div(k.batch, kRowWaves)), dim3(kRowWaves * kWave), 0, k.stream>>>(ra);
    ADX_LAUNCH_CHECK();
    return ADX_OK;
  }
  kernels[k.pin != nullptr][guided]<<<dim3(ceil_div(a.total, 256)), dim3(256), 0, k.stream>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

// What a plan still violates (adx_guide_cost): per row the cost of "cost guidance v1" summed over its waypoints and the number of
// active (waypoint, constraint) pairs.  Shaped like the control kernel: one wave per row, four rows per workgroup, lane = waypoint;
// the waves share nothing (no LDS, no atomics), the two sums are the fixed xor butterfly, lane 0 stores.
constexpr int kCostWaves = 4;

struct GuideCostArgs {
  const float* traj;
  GuideArgs g;
  float* cost;
  int32_t* active;
  int rows, horizon, dim;
  MotionArgs motion;      // cost guidance v3 (the MOTION kernel only)
};

// MOTION ("cost guidance v3"): a waypoint's share of the segment and curvature terms after its v1 / v2 terms; the neighbours'
// xy come by shuffle, so lanes h >= H stay to the end and hold zeros
template <bool MOTION>
__global__ void __launch_bounds__(kCostWaves * kWave) guide_cost_kernel(const GuideCostArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & (kWave - 1);
  const int r = blockIdx.x * kCostWaves + (threadIdx.x >> 6);
  if (r >= a.rows) return;                       // whole waves leave: the shuffles below always see all 64 lanes
  float J = 0.f, gx, gy;
  int active = 0;
  if constexpr (MOTION) {
    const bool live = lane < a.horizon;
    float nx[5], ny[5];
    nx[2] = 0.f; ny[2] = 0.f;
    if (live) {
      const float* p = a.traj + ((size_t)r * a.horizon + lane) * a.dim;
      nx[2] = p[0]; ny[2] = p[1];
    }
    nx[0] = __shfl_up(nx[2], 2, kWave); ny[0] = __shfl_up(ny[2], 2, kWave);
    nx[1] = __shfl_up(nx[2], 1, kWave); ny[1] = __shfl_up(ny[2], 1, kWave);
    nx[3] = __shfl_down(nx[2], 1, kWave); ny[3] = __shfl_down(ny[2], 1, kWave);
    nx[4] = __shfl_down(nx[2], 2, kWave); ny[4] = __shfl_down(ny[2], 2, kWave);
    if (live) {
      float S2, A2;
      motion_limits(a.motion, r, S2, A2);
      guide_grad(scene_guide<true>(a.g, r), (float)lane, nx[2], ny[2], J, gx, gy, active);
      motion_grad(nx, ny, lane, a.horizon, S2, A2, a.motion.w_speed, a.motion.w_accel, J, gx, gy, active);
    }
  } else if (lane < a.horizon) {
    const float* p = a.traj + ((size_t)r * a.horizon + lane) * a.dim;
    guide_grad(scene_guide<true>(a.g, r), (float)lane, p[0], p[1], J, gx, gy, active);
  }
  J = wave_sum(J);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) active += __shfl_xor(active, off, kWave);
  if (lane == 0) {
    a.cost[r] = J;
    a.active[r] = active;
  }
}

int guide_cost(const float* traj, const GuideRecords& g, float* cost, int32_t* active, int rows, int horizon, int dim, hipStream_t s) {
  const char* const what = "guide cost";
  ADX_REQUIRE(traj != nullptr && (g.guide != nullptr || g.field != nullptr) && cost != nullptr && active != nullptr,
              "guide cost: null traj, guide, cost or active");
  ADX_REQUIRE(horizon >= 1 && horizon <= kWave, "guide cost: horizon %d outside 1..%d", horizon, kWave);
  int rc = shape_check(what, rows, horizon, dim);
  if (rc != ADX_OK) return rc;
  GuideCostArgs a;
  const size_t cn = (size_t)rows * sizeof(float);
  const ByteSpan outs[2] = {{cost, cn}, {active, cn}};
  rc = guide_records_check(g, what, false, false, outs, 2, rows, horizon, dim, &a.g, &a.motion);
  if (rc != ADX_OK) return rc;
  const size_t tn = (size_t)rows * horizon * dim * sizeof(float);
  ADX_REQUIRE(!byte_ranges_overlap(cost, cn, traj, tn) && !byte_ranges_overlap(active, cn, traj, tn) &&
              !byte_ranges_overlap(cost, cn, active, cn), "guide cost: an output overlaps traj or the other output");
  a.traj = traj; a.cost = cost; a.active = active; a.rows = rows; a.horizon = horizon; a.dim = dim;
  if (g.motion != nullptr) guide_cost_kernel<true><<<dim3(ceil_div(rows, kCostWaves)), dim3(kCostWaves * kWave), 0, s>>>(a);
  else guide_cost_kernel<false><<<dim3(ceil_div(rows, kCostWaves)), dim3(kCostWaves * kWave), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

// The blend by itself, in place on a sample [batch][H][D]: the entry of a `clean` tick, where the reference writes
// trajs[:, 0, :3] = 0 before its loop.  z, when asked for, is the stream's INIT_SLOT draw of the element's logical index.
struct PinApplyArgs {
  float* x;
  PinArgs pin;
  const uint32_t* ns;
  uint64_t base;
  int total;
};

__global__ void __launch_bounds__(256) pin_apply_kernel(const PinApplyArgs a) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.total) return;
  const float zn = a.pin.known_noise ? noise_normal_at(a.ns, 0xFFFFFFFFu, a.base + (uint64_t)e) : 0.f;
  a.x[e] = pin_blend(a.pin, e, zn, a.x[e]);
}

int pin_apply(float* x, const adx_pin* pin, const uint32_t* ns, int64_t row_offset, int batch, int horizon, int dim, hipStream_t s) {
  const char* const what = "pin apply";
  ADX_REQUIRE(x != nullptr && pin != nullptr, "pin apply: null sample or pin");
  int rc = shape_check(what, batch, horizon, dim);
  if (rc != ADX_OK) return rc;
  PinApplyArgs a;
  rc = pin_check(pin, what, ns != nullptr, x, nullptr, batch, horizon, dim, &a.pin);
  if (rc != ADX_OK) return rc;
  a.ns = nullptr; a.base = 0;
  if (ns != nullptr) {
    rc = noise_rows(what, row_offset, batch, (int64_t)horizon * dim, &a.base);
    if (rc != ADX_OK) return rc;
    a.ns = ns;
  }
  a.x = x; a.total = batch * horizon * dim;
  pin_apply_kernel<<<dim3(ceil_div(a.total, 256)), dim3(256), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

// Fill out[0, n) with the stream's values of the logical elements [first, first + n): what a step kernel draws at those
// elements under the same (state, slot).  One thread per element through the same __device__ function as the step.
template <bool NORMAL, typename T>
__global__ void __launch_bounds__(256) noise_fill_kernel(const uint32_t* state, uint32_t slot, uint64_t first, T* out, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (NORMAL) out[i] = (T)noise_normal_at(state, slot, first + i);
  else out[i] = (T)noise_word_at(state, slot, first + i);
}

template <bool NORMAL, typename T>
static int noise_fill(const uint32_t* state, int32_t slot, int64_t first, T* out, int64_t n, hipStream_t s) {
  ADX_REQUIRE(state != nullptr, "noise fill: null noise state");
  ADX_REQUIRE(first >= 0 && n >= 0, "noise fill: negative first element %lld or count %lld", (long long)first, (long long)n);
  ADX_REQUIRE(first <= kNoiseElems && n <= kNoiseElems - first,
              "noise fill: elements [%lld, %lld + %lld) leave the noise stream's 2^34 elements", (long long)first, (long long)first,
              (long long)n);
  if (n == 0) return ADX_OK;
  ADX_REQUIRE(out != nullptr, "noise fill: null output");
  noise_fill_kernel<NORMAL, T><<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(state, (uint32_t)slot, (uint64_t)first, out,
                                                                                      (uint64_t)n);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

int noise_normal(const uint32_t* state, int32_t slot, int64_t first, float* out, int64_t n, hipStream_t s) {
  return noise_fill<true, float>(state, slot, first, out, n, s);
}
int noise_words(const uint32_t* state, int32_t slot, int64_t first, uint32_t* out, int64_t n, hipStream_t s) {
  return noise_fill<false, uint32_t>(state, slot, first, out, n, s);
}

// tick += 1 (64-bit, two words), by one vector lane: the next launches on the stream draw under the new tick
__global__ void noise_advance_kernel(uint32_t* state) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const uint32_t lo = state[2] + 1u;
  state[2] = lo;
  if (lo == 0u) state[3] = state[3] + 1u;
}

int noise_advance(uint32_t* state, hipStream_t s) {
  ADX_REQUIRE(state != nullptr, "noise advance: null noise state");
  noise_advance_kernel<<<dim3(1), dim3(1), 0, s>>>(state);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

// Warm start v1 (include/adx.h): this tick's initial trajectory from the last tick's result -- advance by `shift` waypoints,
// re-base onto the new first waypoint (or the caller's odometry), clamp, re-noise to the level the schedule's suffix starts at.
// One thread per OUTPUT element; the noise is the stream's INIT_SLOT draw of the element's logical index, as in step_kernel.
struct WarmArgs {
  const float* prev;      // [prev_rows][H][D]
  const float* motion;    // [prev_rows][3] = (tx, ty, phi), or null
  float* out;             // [rows][H][D]
  const uint32_t* ns;
  uint64_t base;          // first logical element of this launch's rows
  float sqrt_ab, sqrt_1mab;
  int total, prev_rows, horizon, dim, shift, zero_first;
};

__global__ void __launch_bounds__(256) warm_init_kernel(const WarmArgs a) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.total) return;
  const int H = a.horizon, D = a.dim;
  const int d = e % D, h = (e / D) % H, r = e / (H * D);
  const int pr = r % a.prev_rows;
  const float* p = a.prev + (size_t)pr * H * D;
  float w;
  if (a.motion != nullptr && d < 2) {
    const float tx = a.motion[pr * 3 + 0], ty = a.motion[pr * 3 + 1], phi = a.motion[pr * 3 + 2];
    const float c = cosf(phi), s = sinf(phi);
    const float qx = warm_advance(p, h, 0, H, D, a.shift) - tx;
    const float qy = (D > 1 ? warm_advance(p, h, 1, H, D, a.shift) : 0.f) - ty;
    if (d == 0) {
      const float m0 = c * qx, m1 = s * qy;
      w = m0 + m1;
    } else {
      const float m0 = s * qx, m1 = c * qy;
      w = -m0 + m1;
    }
  } else {
    w = warm_advance(p, h, d, H, D, a.shift);
    if (d < 3) w = w - p[a.shift * D + d];
  }
  w = clamp_nan(w, -1.0f, 1.0f);
  const float z = noise_normal_at(a.ns, 0xFFFFFFFFu, a.base + (uint64_t)e);
  const float m0 = a.sqrt_ab * w, m1 = a.sqrt_1mab * z;
  float v = m0 + m1;
  if (a.zero_first && first_pose(e, H, D)) v = 0.f;
  a.out[e] = v;
}

int warm_init(const float* prev, int prev_rows, const float* motion, float* out, int rows, int horizon, int dim, int shift,
              float sqrt_ab, float sqrt_1mab, const uint32_t* ns, int64_t row_offset, int zero_first, hipStream_t s) {
  ADX_REQUIRE(prev != nullptr && out != nullptr && ns != nullptr, "warm init: null prev, out or noise state");
  ADX_REQUIRE(horizon >= 2 && horizon <= 64, "warm init: horizon %d outside 2..64", horizon);
  ADX_REQUIRE(dim >= 1 && dim <= 16, "warm init: dim %d outside 1..16", dim);
  ADX_REQUIRE(shift >= 0 && shift <= horizon - 1, "warm init: shift %d outside 0..%d (horizon - 1)", shift, horizon - 1);
  ADX_REQUIRE(prev_rows >= 1 && rows >= 1 && rows % prev_rows == 0, "warm init: rows %d must be a positive multiple of prev_rows %d",
              rows, prev_rows);
  const int64_t per = (int64_t)horizon * dim;
  WarmArgs a;
  int rc = noise_rows("warm init", row_offset, rows, per, &a.base);
  if (rc != ADX_OK) return rc;
  rc = shape_check("warm init", rows, horizon, dim);
  if (rc != ADX_OK) return rc;
  ADX_REQUIRE(!byte_ranges_overlap(out,(size_t)rows * per * sizeof(float), prev, (size_t)prev_rows * per * sizeof(float)),
              "warm init: the output overlaps prev");
  a.prev = prev; a.motion = motion; a.out = out; a.ns = ns;
  a.sqrt_ab = sqrt_ab; a.sqrt_1mab = sqrt_1mab;
  a.total = (int)(rows * per); a.prev_rows = prev_rows; a.horizon = horizon; a.dim = dim; a.shift = shift;
  a.zero_first = zero_first != 0;
  warm_init_kernel<<<dim3(ceil_div(a.total, 256)), dim3(256), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

__global__ void __launch_bounds__(256) add_noise_kernel(const float* __restrict__ x, const float* __restrict__ n,
                                                         const int64_t* __restrict__ t, const float* __restrict__ sa,
                                                         const float* __restrict__ sb, float* __restrict__ out,
                                                         int total, int per, int horizon, int dim, int zero_first) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int b = e / per;
  const int64_t tb = t[b];
  const float p = sa[tb] * x[e], q = sb[tb] * n[e];
  float v = p + q;
  if (zero_first && first_pose(e, horizon, dim)) v = 0.f;
  out[e] = v;
}

int add_noise(const float* x, const float* n, const int64_t* t, const float* sa, const float* sb, int n_train,
              float* out, int batch, int horizon, int dim, int zero_first, hipStream_t s) {
  ADX_REQUIRE(x && n && t && sa && sb && out, "add_noise: null tensor");
  ADX_REQUIRE(n_train >= 1, "add_noise: empty shape");
  const int rc = shape_check("add_noise", batch, horizon, dim);
  if (rc != ADX_OK) return rc;
  const int total = batch * horizon * dim;
  add_noise_kernel<<<dim3(ceil_div(total, 256)), dim3(256), 0, s>>>(x, n, t, sa, sb, out, total, horizon * dim,
                                                                  horizon, dim, zero_first);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

// Camera front-end of the agents (interact.py:73-78, e2e_driving/diffusion_agent.py:96-101,294):
// torchvision ToTensor + Normalize(mean, std) on a uint8 HWC frame -> fp32 NCHW, one pass.
__global__ void __launch_bounds__(256) image_normalize_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst,
                                                               int n, int h, int w, float m0, float m1, float m2,
                                                               float s0, float s1, float s2) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;   // one output pixel (all 3 channels)
  const size_t hw = (size_t)h * w;
  if (i >= (size_t)n * hw) return;
  const size_t img = i / hw, pix = i - img * hw;
  const uint8_t* p = src + i * 3;
  const float mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = (float)p[c] / 255.0f;              // ToTensor
    dst[(img * 3 + c) * hw + pix] = (v - mean[c]) / stdv[c];
  }
}

int image_normalize(const uint8_t* src, float* dst, int n, int h, int w, const float* mean, const float* stdv,
                    hipStream_t s) {
  ADX_REQUIRE(src && dst && mean && stdv && n >= 1 && h >= 1 && w >= 1, "image_normalize: bad argument");
  const size_t total = (size_t)n * h * w;
  image_normalize_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s>>>(src, dst, n, h, w, mean[0], mean[1],
                                                                                  mean[2], stdv[0], stdv[1], stdv[2]);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

}  // namespace adx
