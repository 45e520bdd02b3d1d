// Host-only check of the entry point of csrc/expert.hip: every refusal of expert_plan, each of which returns before any GPU
// work.  Built together with the source by tests/test_expert_host.py with the host side under AddressSanitizer and UBSan, and run
// as a program of its own: it needs no GPU (nothing is launched) and is not loaded into Python.  Exit status 0 = every check held.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

// by its path: a -I of csrc/ would put this sched.h in front of the system's <sched.h>
#include "../../autonomous_driving_with_diffusion_model_amd/csrc/sched.h"

static char g_error[512];

namespace adx {
void set_error(const char* fmt, ...) {      // api.cpp's, without the library around it
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}
}  // namespace adx

extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }      // the HIP runtime's own start-up allocations

static int g_failed = 0;

static void expect(bool ok, const char* what) {
  if (!ok) {
    fprintf(stderr, "FAILED: %s (last error: %s)\n", what, g_error);
    ++g_failed;
  }
}

static void refused(int rc, const char* text, const char* what) {
  expect(rc == ADX_ERR_INVALID && strstr(g_error, text) != nullptr, what);
  g_error[0] = 0;
}

int main() {
  using namespace adx;
  const int S = 2, R = 16, N = 3, M = 2, K = 4, H = 16, D = 7;
  adx_expert_cfg good = {};
  good.scenes = S; good.window = R; good.n_boxes = N; good.n_discs = M; good.n_planes = K; good.horizon = H; good.dim = D;
  good.xy_scale = 23.315; good.waypoint_dt = 0.5; good.desired_v = 8.0; good.accel = 1.5; good.brake = 2.0; good.brake_max = 8.0;
  good.headway = 1.5; good.jam = 2.0; good.gap_min = 0.25; good.corridor_half = 1.75; good.lat_accel = 2.0; good.look_time = 2.0;
  good.ego_front = 2.25; good.end_margin = 1.0; good.look_min = 10.0;

  // host memory stands in for device memory: no refusal dereferences a pointer
  // (each with room for the largest output behind it, so that an output laid into one overlaps that one alone)
  const size_t room = S * H * D;
  std::vector<float> window(S * R * 2 + room), velocity(S + room), boxes(S * N * 8 + room), discs(S * M * 5 + room), planes(S * K * 3 + room),
      plan(S * H * D + room), info(S * 8 + room);
  std::vector<int32_t> leader(S + room);
  float* const W = window.data(); float* const V = velocity.data(); float* const B = boxes.data(); float* const C = discs.data();
  float* const P = planes.data(); float* const T = plan.data(); float* const I = info.data(); int32_t* const L = leader.data();
  auto run = [&](const adx_expert_cfg& k) { return expert_plan(&k, W, V, B, C, P, T, L, I, nullptr); };
  adx_expert_cfg c;

  refused(expert_plan(nullptr, W, V, B, C, P, T, L, I, nullptr), "null configuration", "expert: null cfg");
  c = good; c.scenes = 0; refused(run(c), "0 scenes", "expert: scenes");
  c = good; c.scenes = 65536; refused(run(c), "65536 scenes", "expert: scenes high");
  c = good; c.window = 1; refused(run(c), "1 window points", "expert: window");
  c = good; c.window = 33; refused(run(c), "33 window points", "expert: window high");
  c = good; c.n_boxes = -1; refused(run(c), "-1 boxes", "expert: boxes");
  c = good; c.n_boxes = 65; refused(run(c), "65 boxes", "expert: boxes high");
  c = good; c.n_discs = -1; refused(run(c), "-1 discs", "expert: discs");
  c = good; c.n_discs = 65; refused(run(c), "65 discs", "expert: discs high");
  c = good; c.n_planes = -1; refused(run(c), "-1 planes", "expert: planes");
  c = good; c.n_planes = 9; refused(run(c), "9 planes", "expert: planes high");
  c = good; c.horizon = 1; refused(run(c), "horizon 1", "expert: horizon");
  c = good; c.horizon = 65; refused(run(c), "horizon 65", "expert: horizon high");
  c = good; c.dim = 1; refused(run(c), "dim 1", "expert: dim");
  c = good; c.dim = 17; refused(run(c), "dim 17", "expert: dim high");
  {
    double adx_expert_cfg::*const pos[12] = {&adx_expert_cfg::xy_scale, &adx_expert_cfg::waypoint_dt, &adx_expert_cfg::desired_v,
                                            &adx_expert_cfg::accel, &adx_expert_cfg::brake, &adx_expert_cfg::brake_max,
                                            &adx_expert_cfg::headway, &adx_expert_cfg::jam, &adx_expert_cfg::gap_min,
                                            &adx_expert_cfg::corridor_half, &adx_expert_cfg::lat_accel, &adx_expert_cfg::look_time};
    const char* const names[12] = {"xy_scale", "waypoint_dt", "desired_v", "accel", "brake", "brake_max", "headway", "jam", "gap_min",
                                   "corridor_half", "lat_accel", "look_time"};
    const double bad[4] = {0.0, -1.0, __builtin_inf(), __builtin_nan("")};
    for (int i = 0; i < 12; ++i)
      for (int j = 0; j < 4; ++j) {
        char text[64], what[64];
        snprintf(text, sizeof(text), "%s %g must be finite and > 0", names[i], bad[j]);
        snprintf(what, sizeof(what), "expert: %s = %g", names[i], bad[j]);
        c = good; c.*pos[i] = bad[j]; refused(run(c), text, what);
      }
    double adx_expert_cfg::*const non[3] = {&adx_expert_cfg::ego_front, &adx_expert_cfg::end_margin, &adx_expert_cfg::look_min};
    const char* const non_names[3] = {"ego_front", "end_margin", "look_min"};
    const double worse[3] = {-0.5, __builtin_inf(), __builtin_nan("")};
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        char text[64], what[64];
        snprintf(text, sizeof(text), "%s %g must be finite and >= 0", non_names[i], worse[j]);
        snprintf(what, sizeof(what), "expert: %s = %g", non_names[i], worse[j]);
        c = good; c.*non[i] = worse[j]; refused(run(c), text, what);
      }
  }
#define PLAN(WIN, VEL, BOX, DISC, PLANE, OUT, LEAD, INFO) expert_plan(&good, WIN, VEL, BOX, DISC, PLANE, OUT, LEAD, INFO, nullptr)
  refused(PLAN(nullptr, V, B, C, P, T, L, I), "null window", "expert: null window");
  refused(PLAN(W, nullptr, B, C, P, T, L, I), "null velocity", "expert: null velocity");
  refused(PLAN(W, V, nullptr, C, P, T, L, I), "boxes must be given exactly when n_boxes > 0 (3)", "expert: null boxes");
  refused(PLAN(W, V, B, nullptr, P, T, L, I), "discs must be given exactly when n_discs > 0 (2)", "expert: null discs");
  refused(PLAN(W, V, B, C, nullptr, T, L, I), "planes must be given exactly when n_planes > 0 (4)", "expert: null planes");
  refused(PLAN(W, V, B, C, P, nullptr, L, I), "null plan", "expert: null plan");
  refused(PLAN(W, V, B, C, P, T, nullptr, I), "null leader", "expert: null leader");
  refused(PLAN(W, V, B, C, P, T, L, nullptr), "null info", "expert: null info");
  c = good; c.n_boxes = 0; refused(run(c), "boxes must be given exactly when n_boxes > 0 (0)", "expert: boxes without a count");
  c = good; c.n_discs = 0; refused(run(c), "discs must be given exactly when n_discs > 0 (0)", "expert: discs without a count");
  c = good; c.n_planes = 0; refused(run(c), "planes must be given exactly when n_planes > 0 (0)", "expert: planes without a count");
  // an output on an input
  refused(PLAN(W, V, B, C, P, W, L, I), "plan aliases window", "expert: plan on window");
  refused(PLAN(W, V, B, C, P, B + 3, L, I), "plan aliases boxes", "expert: plan in boxes");
  refused(PLAN(W, V, B, C, P, C, L, I), "plan aliases discs", "expert: plan on discs");
  refused(PLAN(W, V, B, C, P, P, L, I), "plan aliases planes", "expert: plan on planes");
  refused(PLAN(W, V, B, C, P, T, reinterpret_cast<int32_t*>(V), I), "leader aliases velocity", "expert: leader on velocity");
  refused(PLAN(W, V, B, C, P, T, L, W + 8), "info aliases window", "expert: info in window");
  refused(PLAN(W, V, B, C, P, T, L, P + S * K * 3 - 1), "info aliases planes", "expert: info on the last word of planes");
  // an output on another output
  refused(PLAN(W, V, B, C, P, T, reinterpret_cast<int32_t*>(T + 5), I), "plan and leader alias each other", "expert: leader in plan");
  refused(PLAN(W, V, B, C, P, T, L, T + S * H * D - 1), "plan and info alias each other", "expert: info on the last word of plan");
  refused(PLAN(W, V, B, C, P, T, L, reinterpret_cast<float*>(L)), "leader and info alias each other", "expert: info on leader");

  // the edges of every range with an empty world pass the checks up to the first pointer: what is refused next is the null window
  c = good; c.scenes = 65535; c.window = 32; c.n_boxes = c.n_discs = c.n_planes = 0; c.horizon = 64; c.dim = 16;
  c.ego_front = c.end_margin = c.look_min = 0.0;
  refused(expert_plan(&c, nullptr, V, nullptr, nullptr, nullptr, T, L, I, nullptr), "null window", "expert: the edges of the ranges, then null window");
  c.window = 2; c.horizon = 2; c.dim = 2; c.scenes = 1;
  refused(expert_plan(&c, nullptr, V, nullptr, nullptr, nullptr, T, L, I, nullptr), "null window", "expert: the low edges, then null window");

  if (g_failed == 0) printf("expert host check: every refusal held\n");
  return g_failed == 0 ? 0 : 1;
}
