// Host-only check of the entry points of csrc/traffic.hip: traffic_state_bytes and every refusal of traffic_step and
// traffic_reset, each of which returns before any GPU work.  Built together with the source by tests/test_traffic_host.py with
// the host side under AddressSanitizer and UBSan, and run as a program of its own: it needs no GPU (nothing is launched) and is
// not loaded into Python.  Exit status 0 = every check held.
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
  expect(traffic_state_bytes(1, 1) == 4u * 38u && traffic_state_bytes(3, 5) == 3u * 4u * 58u && traffic_state_bytes(1, 64) == 4u * 352u &&
             traffic_state_bytes(65535, 64) == 65535u * 4u * 352u,
         "traffic_state_bytes");
  expect(traffic_state_bytes(0, 5) == 0 && traffic_state_bytes(-3, 5) == 0 && traffic_state_bytes(65536, 5) == 0 &&
             traffic_state_bytes(3, 0) == 0 && traffic_state_bytes(3, 65) == 0,
         "traffic_state_bytes out of range");

  // host memory stands in for device memory: no refusal dereferences a pointer
  const int S = 3, N = 5, Q = 2, G = 7, T = 3, NS = 4;
  std::vector<double> paths(S * Q * G * 2), cum(S * Q * G), heading(S * Q * G), agents(S * N * 9), stops(S * T * 3), pose(S * 3),
      boxes(S * N * 7);
  std::vector<int32_t> plen(S * Q), phase(S * NS), hold(S), leader(S * N);
  std::vector<float> velocity(S);
  std::vector<uint8_t> state(traffic_state_bytes(S, N)), mask(S);

  const adx_traffic_cfg good = {S, N, Q, G, T, NS, 0.1, 1.75, 4.5, 2.0, 0.25, 8.0};
  struct Ptrs {
    const double *paths, *cum, *heading, *agents, *stops, *pose;
    const int32_t *plen, *phase, *hold;
    const float* velocity;
    void* state;
    double* boxes;
    int32_t* leader;
    const uint8_t* mask;
  };
  const Ptrs all = {paths.data(), cum.data(),  heading.data(),  agents.data(), stops.data(), pose.data(),   plen.data(),
                    phase.data(), hold.data(), velocity.data(), state.data(),  boxes.data(), leader.data(), mask.data()};
  auto step = [&](const adx_traffic_cfg& c, const Ptrs& p) {
    return traffic_step(&c, p.paths, p.plen, p.cum, p.heading, p.agents, p.stops, p.phase, p.pose, p.velocity, p.hold, p.state, p.boxes,
                        p.leader, nullptr);
  };
  auto reset = [&](const adx_traffic_cfg& c, const Ptrs& p) {
    return traffic_reset(&c, p.paths, p.plen, p.cum, p.heading, p.agents, p.mask, p.state, p.boxes, p.leader, nullptr);
  };
  adx_traffic_cfg c = good;
  Ptrs p = all;
  refused(traffic_step(nullptr, p.paths, p.plen, p.cum, p.heading, p.agents, p.stops, p.phase, p.pose, p.velocity, p.hold, p.state, p.boxes,
                       p.leader, nullptr),
          "traffic step: null configuration", "traffic step: null cfg");
  // the limits
  c = good; c.scenes = 0; refused(step(c, all), "0 scenes", "traffic step: scenes");
  c = good; c.scenes = 65536; refused(step(c, all), "65536 scenes", "traffic step: scenes high");
  c = good; c.n_agents = 0; refused(step(c, all), "0 agents", "traffic step: agents");
  c = good; c.n_agents = 65; refused(step(c, all), "65 agents", "traffic step: agents high");
  c = good; c.n_paths = 0; refused(step(c, all), "0 paths", "traffic step: paths");
  c = good; c.n_paths = 9; refused(step(c, all), "9 paths", "traffic step: paths high");
  c = good; c.n_points = 1; refused(step(c, all), "1 path points", "traffic step: points");
  c = good; c.n_points = 65; refused(step(c, all), "65 path points", "traffic step: points high");
  c = good; c.n_stops = -1; refused(step(c, all), "-1 stops", "traffic step: stops");
  c = good; c.n_stops = 17; refused(step(c, all), "17 stops", "traffic step: stops high");
  c = good; c.n_signals = 0; refused(step(c, all), "0 signals", "traffic step: signals with stops");
  c = good; c.n_signals = 65; refused(step(c, all), "65 signals", "traffic step: signals high");
  c = good; c.n_stops = 0; c.n_signals = -1; refused(step(c, all), "-1 signals", "traffic step: signals negative");
  // the configuration's numbers
  c = good; c.dt = 0.0; refused(step(c, all), "dt 0", "traffic step: dt");
  c = good; c.dt = __builtin_nan(""); refused(step(c, all), "dt nan", "traffic step: dt nan");
  c = good; c.dt = __builtin_inf(); refused(step(c, all), "dt inf", "traffic step: dt inf");
  c = good; c.lane_half_width = -1.0; refused(step(c, all), "lane_half_width -1", "traffic step: lane_half_width");
  c = good; c.lane_half_width = __builtin_nan(""); refused(step(c, all), "lane_half_width nan", "traffic step: lane_half_width nan");
  c = good; c.ego_length = 0.0; refused(step(c, all), "ego_length 0", "traffic step: ego_length");
  c = good; c.ego_length = __builtin_inf(); refused(step(c, all), "ego_length inf", "traffic step: ego_length inf");
  c = good; c.jam = 0.0; refused(step(c, all), "jam 0", "traffic step: jam");
  c = good; c.jam = __builtin_nan(""); refused(step(c, all), "jam nan", "traffic step: jam nan");
  c = good; c.gap_min = 0.0; refused(step(c, all), "gap_min 0", "traffic step: gap_min");
  c = good; c.gap_min = -0.25; refused(step(c, all), "gap_min -0.25", "traffic step: gap_min negative");
  c = good; c.brake_max = -8.0; refused(step(c, all), "brake_max -8", "traffic step: brake_max");
  c = good; c.brake_max = __builtin_inf(); refused(step(c, all), "brake_max inf", "traffic step: brake_max inf");
  // the NULLs; first with every range at its edge, which is in range
  c = good; c.n_agents = 64; c.n_paths = 8; c.n_points = 64; c.n_stops = 16; c.n_signals = 64; c.scenes = 1;
  p = all; p.paths = nullptr; refused(step(c, p), "null paths", "traffic step: the edges of every range, then null paths");
  p = all; p.plen = nullptr; refused(step(good, p), "null plen", "traffic step: null plen");
  p = all; p.cum = nullptr; refused(step(good, p), "null cum", "traffic step: null cum");
  p = all; p.heading = nullptr; refused(step(good, p), "null heading", "traffic step: null heading");
  p = all; p.agents = nullptr; refused(step(good, p), "null agents", "traffic step: null agents");
  p = all; p.pose = nullptr; refused(step(good, p), "null pose", "traffic step: null pose");
  p = all; p.velocity = nullptr; refused(step(good, p), "null velocity", "traffic step: null velocity");
  p = all; p.state = nullptr; refused(step(good, p), "null state", "traffic step: null state");
  p = all; p.boxes = nullptr; refused(step(good, p), "null boxes", "traffic step: null boxes");
  p = all; p.leader = nullptr; refused(step(good, p), "null leader", "traffic step: null leader");
  p = all; p.stops = nullptr; refused(step(good, p), "stops must be given exactly when n_stops > 0 (3)", "traffic step: stops missing");
  p = all; p.phase = nullptr; refused(step(good, p), "phase must be given exactly when n_stops > 0 (3)", "traffic step: phase missing");
  c = good; c.n_stops = 0; c.n_signals = 0;
  p = all; p.phase = nullptr; refused(step(c, p), "stops must be given exactly when n_stops > 0 (0)", "traffic step: stops without a count");
  p = all; p.stops = nullptr; refused(step(c, p), "phase must be given exactly when n_stops > 0 (0)", "traffic step: phase without a count");
  // an output on an input, every input once
  p = all; p.state = paths.data() + 4; refused(step(good, p), "the state aliases paths", "traffic step: the state on paths");
  p = all; p.boxes = reinterpret_cast<double*>(plen.data()); refused(step(good, p), "boxes aliases plen", "traffic step: boxes on plen");
  p = all; p.leader = reinterpret_cast<int32_t*>(cum.data() + 1); refused(step(good, p), "leader aliases cum", "traffic step: leader on cum");
  p = all; p.state = heading.data(); refused(step(good, p), "the state aliases heading", "traffic step: the state on heading");
  p = all; p.boxes = agents.data() + 9; refused(step(good, p), "boxes aliases agents", "traffic step: boxes on agents");
  p = all; p.leader = reinterpret_cast<int32_t*>(stops.data()); refused(step(good, p), "leader aliases stops", "traffic step: leader on stops");
  p = all; p.leader = phase.data(); refused(step(good, p), "leader aliases phase", "traffic step: leader on phase");
  p = all; p.boxes = pose.data(); refused(step(good, p), "boxes aliases pose", "traffic step: boxes on pose");
  p = all; p.leader = reinterpret_cast<int32_t*>(velocity.data()); refused(step(good, p), "leader aliases velocity", "traffic step: leader on velocity");
  p = all; p.hold = reinterpret_cast<const int32_t*>(state.data() + 8); refused(step(good, p), "the state aliases hold", "traffic step: hold in the state");
  // an output on another
  p = all; p.boxes = reinterpret_cast<double*>(state.data() + 64); refused(step(good, p), "the state and boxes alias each other", "traffic step: boxes in the state");
  p = all; p.leader = reinterpret_cast<int32_t*>(state.data() + state.size() - 60);
  refused(step(good, p), "the state and leader alias each other", "traffic step: leader on the state's last words");
  p = all; p.leader = reinterpret_cast<int32_t*>(boxes.data() + 3); refused(step(good, p), "boxes and leader alias each other", "traffic step: leader in boxes");
  // the reset
  refused(traffic_reset(nullptr, all.paths, all.plen, all.cum, all.heading, all.agents, nullptr, all.state, all.boxes, all.leader, nullptr),
          "traffic reset: null configuration", "traffic reset: null cfg");
  c = good; c.scenes = 0; refused(reset(c, all), "traffic reset: 0 scenes", "traffic reset: scenes");
  c = good; c.scenes = 65536; refused(reset(c, all), "65536 scenes", "traffic reset: scenes high");
  c = good; c.n_agents = 65; refused(reset(c, all), "65 agents", "traffic reset: agents");
  c = good; c.n_paths = 9; refused(reset(c, all), "9 paths", "traffic reset: paths");
  c = good; c.n_points = 1; refused(reset(c, all), "1 path points", "traffic reset: points");
  c = good; c.dt = -1.0; refused(reset(c, all), "dt -1", "traffic reset: dt");
  p = all; p.paths = nullptr; refused(reset(good, p), "null paths", "traffic reset: null paths");
  p = all; p.agents = nullptr; refused(reset(good, p), "null agents", "traffic reset: null agents");
  p = all; p.state = nullptr; refused(reset(good, p), "null state", "traffic reset: null state");
  p = all; p.boxes = nullptr; refused(reset(good, p), "null boxes", "traffic reset: null boxes");
  p = all; p.mask = state.data() + 5; refused(reset(good, p), "the state aliases the mask", "traffic reset: the mask in the state");
  p = all; p.mask = reinterpret_cast<const uint8_t*>(boxes.data()); refused(reset(good, p), "boxes aliases the mask", "traffic reset: the mask in boxes");
  p = all; p.mask = reinterpret_cast<const uint8_t*>(leader.data()) + 1; refused(reset(good, p), "leader aliases the mask", "traffic reset: the mask in leader");
  p = all; p.boxes = reinterpret_cast<double*>(state.data()); refused(reset(good, p), "the state and boxes alias each other", "traffic reset: boxes on the state");
  p = all; p.leader = reinterpret_cast<int32_t*>(agents.data()); refused(reset(good, p), "leader aliases agents", "traffic reset: leader on agents");
  p = all; p.state = cum.data(); refused(reset(good, p), "the state aliases cum", "traffic reset: the state on cum");

  if (g_failed == 0) printf("traffic host check: every refusal held\n");
  return g_failed == 0 ? 0 : 1;
}
