// Host-only check of the entry points of csrc/signals.hip: signals_state_bytes and every refusal of signals_step and
// signals_reset, each of which returns before any GPU work.  Built together with the source by tests/test_signals_host.py with
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
  expect(signals_state_bytes(1) == 64 && signals_state_bytes(65535) == 64u * 65535u, "signals_state_bytes");
  expect(signals_state_bytes(0) == 0 && signals_state_bytes(-3) == 0 && signals_state_bytes(65536) == 0, "signals_state_bytes out of range");

  // host memory stands in for device memory: no refusal dereferences a pointer
  const int S = 3, N = 5, P = 2;
  std::vector<double> signals(S * N * 10), pose(S * 3);
  std::vector<float> velocity(S), planes(S * P * 3);
  std::vector<int32_t> hold(S), phase(S * N);
  std::vector<uint8_t> state(signals_state_bytes(S)), mask(S);

  const adx_signals_cfg good = {S, N, P, 0, 0.5, 23.315, 3.0, -2.0, 0.0, 0.1};
  auto step = [&](const adx_signals_cfg& c) {
    return signals_step(&c, signals.data(), pose.data(), velocity.data(), hold.data(), state.data(), planes.data(), phase.data(), nullptr);
  };
  adx_signals_cfg c = good;
  refused(signals_step(nullptr, signals.data(), pose.data(), velocity.data(), nullptr, state.data(), planes.data(), phase.data(), nullptr),
          "null configuration", "signals step: null cfg");
  c = good; c.scenes = 0; refused(step(c), "0 scenes", "signals step: scenes");
  c = good; c.scenes = 65536; refused(step(c), "65536 scenes", "signals step: scenes high");
  c = good; c.n_signals = 0; refused(step(c), "0 signals", "signals step: signals");
  c = good; c.n_signals = 65; refused(step(c), "65 signals", "signals step: signals high");
  c = good; c.n_planes = 0; refused(step(c), "0 planes", "signals step: planes");
  c = good; c.n_planes = 9; refused(step(c), "9 planes", "signals step: planes high");
  c = good; c.dt = 0.0; refused(step(c), "dt 0", "signals step: dt");
  c = good; c.dt = __builtin_nan(""); refused(step(c), "dt nan", "signals step: dt nan");
  c = good; c.xy_scale = -1.0; refused(step(c), "xy_scale -1", "signals step: xy_scale");
  c = good; c.xy_scale = __builtin_inf(); refused(step(c), "xy_scale inf", "signals step: xy_scale inf");
  c = good; c.margin = -0.5; refused(step(c), "margin -0.5", "signals step: margin");
  c = good; c.margin = __builtin_nan(""); refused(step(c), "margin nan", "signals step: margin nan");
  c = good; c.probe = __builtin_inf(); refused(step(c), "probe inf", "signals step: probe");
  c = good; c.probe = __builtin_nan(""); refused(step(c), "probe nan", "signals step: probe nan");
  c = good; c.min_cos = 1.0; refused(step(c), "min_cos 1", "signals step: min_cos");
  c = good; c.min_cos = -1.25; refused(step(c), "min_cos -1.25", "signals step: min_cos low");
  c = good; c.min_cos = __builtin_nan(""); refused(step(c), "min_cos nan", "signals step: min_cos nan");
  c = good; c.speed_threshold = -1.0; refused(step(c), "speed_threshold -1", "signals step: speed_threshold");
  c = good; c.speed_threshold = __builtin_inf(); refused(step(c), "speed_threshold inf", "signals step: speed_threshold inf");
  c = good; c.min_cos = -1.0; c.probe = 0.0; c.margin = 0.0; c.speed_threshold = 0.0; c.n_signals = 64; c.n_planes = 8;      // the edges are in range:
  refused(signals_step(&c, nullptr, pose.data(), velocity.data(), nullptr, state.data(), planes.data(), phase.data(), nullptr), "null signals",
          "signals step: the edges of every range, then null signals");
  refused(signals_step(&good, signals.data(), nullptr, velocity.data(), nullptr, state.data(), planes.data(), phase.data(), nullptr), "null pose",
          "signals step: null pose");
  refused(signals_step(&good, signals.data(), pose.data(), nullptr, nullptr, state.data(), planes.data(), phase.data(), nullptr), "null velocity",
          "signals step: null velocity");
  refused(signals_step(&good, signals.data(), pose.data(), velocity.data(), nullptr, nullptr, planes.data(), phase.data(), nullptr), "null state",
          "signals step: null state");
  refused(signals_step(&good, signals.data(), pose.data(), velocity.data(), nullptr, state.data(), nullptr, phase.data(), nullptr), "null planes",
          "signals step: null planes");
  refused(signals_step(&good, signals.data(), pose.data(), velocity.data(), nullptr, state.data(), planes.data(), nullptr, nullptr), "null phase",
          "signals step: null phase");
  refused(signals_step(&good, signals.data(), pose.data(), velocity.data(), hold.data(), signals.data() + 4, planes.data(), phase.data(), nullptr),
          "the state aliases signals", "signals step: the state on an input");
  refused(signals_step(&good, signals.data(), pose.data(), velocity.data(), hold.data(), state.data(), reinterpret_cast<float*>(pose.data()),
                       phase.data(), nullptr),
          "planes aliases pose", "signals step: planes on an input");
  refused(signals_step(&good, signals.data(), pose.data(), velocity.data(), hold.data(), state.data(), planes.data(), hold.data(), nullptr),
          "phase aliases hold", "signals step: phase on hold");
  refused(signals_step(&good, signals.data(), pose.data(), velocity.data(), hold.data(), state.data(), velocity.data(), phase.data(), nullptr),
          "planes aliases velocity", "signals step: planes on velocity");
  refused(signals_step(&good, signals.data(), pose.data(), velocity.data(), hold.data(), state.data(), reinterpret_cast<float*>(state.data() + 64),
                       phase.data(), nullptr),
          "the state and planes alias each other", "signals step: planes in the state");
  refused(signals_step(&good, signals.data(), pose.data(), velocity.data(), hold.data(), state.data(), planes.data(),
                       reinterpret_cast<int32_t*>(planes.data() + 1), nullptr),
          "planes and phase alias each other", "signals step: phase in planes");
  refused(signals_reset(nullptr, S, nullptr, nullptr, 0, nullptr), "null state", "signals reset: null state");
  refused(signals_reset(state.data(), 0, nullptr, nullptr, 0, nullptr), "0 scenes", "signals reset: scenes");
  refused(signals_reset(state.data(), 65536, nullptr, nullptr, 0, nullptr), "65536 scenes", "signals reset: scenes high");
  refused(signals_reset(state.data(), S, nullptr, planes.data(), 0, nullptr), "0 planes", "signals reset: planes");
  refused(signals_reset(state.data(), S, nullptr, planes.data(), 9, nullptr), "9 planes", "signals reset: planes high");
  refused(signals_reset(state.data(), S, state.data() + 4, nullptr, 0, nullptr), "the mask overlaps the state", "signals reset: the mask in the state");
  refused(signals_reset(state.data(), S, nullptr, reinterpret_cast<float*>(state.data()), P, nullptr), "planes_out overlaps the state",
          "signals reset: planes in the state");
  refused(signals_reset(state.data(), S, reinterpret_cast<const uint8_t*>(planes.data()), planes.data(), P, nullptr), "the mask overlaps planes_out",
          "signals reset: the mask in planes");

  if (g_failed == 0) printf("signals host check: every refusal held\n");
  return g_failed == 0 ? 0 : 1;
}
