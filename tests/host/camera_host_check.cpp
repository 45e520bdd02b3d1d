// Host-only check of the entry points of csrc/camera.hip: the arithmetic of camera_prims_bytes, the default palette, and every
// refusal of camera_render, each of which returns before any GPU work.  Built together with the source by
// tests/test_camera_host.py with the host side under AddressSanitizer and UBSan, and run as a program of its own: it needs no GPU
// (nothing is launched) and is not loaded into Python.  Exit status 0 = every check held.
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
  const int S = 2, W = 24, H = 16, NB = 3, ND = 2, NS = 2, Q = 2, G = 4;
  adx_camera_cfg good = {};
  good.scenes = S; good.width = W; good.height = H; good.n_boxes = NB; good.n_discs = ND; good.n_signals = NS; good.n_paths = Q;
  good.n_points = G;
  good.fov = 1.7453292519943295; good.mount_back = -1.5; good.cam_height = 2.0; good.near = 0.1; good.far = 150.0;
  good.half_width = 1.75; good.mark = 0.15; good.line_half = 0.2; good.box_height = 1.6; good.disc_height = 1.8;
  good.lamp_radius = 0.35; good.lamp_height = 4.0; good.lamp_setback = 12.0; good.pole_radius = 0.1;
  for (int i = 0; i < 3; ++i) {
    good.mean[i] = 0.5f;
    good.stdv[i] = 0.25f;
  }
  camera_default_palette(&good.palette[0][0], good.shade);
  expect(good.palette[0][0] == 135 && good.palette[19][2] == 20 && good.shade[4] == 255, "the default palette");
  camera_default_palette(nullptr, nullptr);

  // ---- camera_prims_bytes: 4 * scenes * (16 + 16 n_obj + 8 n_gnd) ----
  const size_t words = 16 + 16 * (NB + ND + 2 * NS) + 8 * (NS + Q * (G - 1));
  expect(camera_prims_bytes(&good) == 4 * S * words, "camera_prims_bytes");
  adx_camera_cfg c = good;
  c.n_boxes = c.n_discs = c.n_signals = c.n_paths = c.n_points = 0;
  expect(camera_prims_bytes(&c) == 4u * S * 16u, "camera_prims_bytes of an empty world");
  c = good; c.scenes = 65535; c.n_boxes = c.n_discs = c.n_signals = 64; c.n_paths = 8; c.n_points = 64;
  expect(camera_prims_bytes(&c) == 4ull * 65535ull * (16 + 16 * 256 + 8 * (64 + 8 * 63)), "camera_prims_bytes at the limits");
  expect(camera_prims_bytes(nullptr) == 0, "camera_prims_bytes of null");
  c = good; c.scenes = 0; expect(camera_prims_bytes(&c) == 0, "camera_prims_bytes: scenes");
  c = good; c.n_boxes = 65; expect(camera_prims_bytes(&c) == 0, "camera_prims_bytes: boxes");
  c = good; c.n_discs = -1; expect(camera_prims_bytes(&c) == 0, "camera_prims_bytes: discs");
  c = good; c.n_signals = 65; expect(camera_prims_bytes(&c) == 0, "camera_prims_bytes: signals");
  c = good; c.n_paths = 9; expect(camera_prims_bytes(&c) == 0, "camera_prims_bytes: paths");
  c = good; c.n_points = 1; expect(camera_prims_bytes(&c) == 0, "camera_prims_bytes: points");
  c = good; c.n_paths = 0; expect(camera_prims_bytes(&c) == 0, "camera_prims_bytes: points without paths");

  // host memory stands in for device memory: no refusal dereferences a pointer
  std::vector<double> pose(S * 3), boxes(S * NB * 7), discs(S * ND * 5), signals(S * NS * 10), roads(S * Q * G * 2);
  std::vector<int32_t> phase(S * NS), road_len(S * Q), hold(S), ids(S * H * W);
  std::vector<float> prims_store(S * words + 4), image(S * 3 * H * W), depth(S * H * W);
  std::vector<uint8_t> frames(S * H * W * 3);
  float* prims = prims_store.data();
  while ((reinterpret_cast<uintptr_t>(prims) & 15u) != 0) ++prims;
  auto render = [&](const adx_camera_cfg& k) {
    return camera_render(&k, pose.data(), boxes.data(), discs.data(), signals.data(), phase.data(), roads.data(), road_len.data(), hold.data(),
                         prims, frames.data(), image.data(), ids.data(), depth.data(), nullptr);
  };
  refused(camera_render(nullptr, pose.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, prims, frames.data(), nullptr, nullptr,
                        nullptr, nullptr),
          "null configuration", "camera: null cfg");
  c = good; c.scenes = 0; refused(render(c), "0 scenes", "camera: scenes");
  c = good; c.scenes = 65536; refused(render(c), "65536 scenes", "camera: scenes high");
  c = good; c.width = 7; refused(render(c), "width 7", "camera: width");
  c = good; c.width = 2049; refused(render(c), "width 2049", "camera: width high");
  c = good; c.height = 7; refused(render(c), "height 7", "camera: height");
  c = good; c.height = 1025; refused(render(c), "height 1025", "camera: height high");
  c = good; c.n_boxes = -1; refused(render(c), "-1 boxes", "camera: boxes");
  c = good; c.n_boxes = 65; refused(render(c), "65 boxes", "camera: boxes high");
  c = good; c.n_discs = 65; refused(render(c), "65 discs", "camera: discs high");
  c = good; c.n_signals = 65; refused(render(c), "65 signals", "camera: signals high");
  c = good; c.n_paths = 9; refused(render(c), "9 paths", "camera: paths high");
  c = good; c.n_points = 1; refused(render(c), "1 points per path", "camera: points");
  c = good; c.n_points = 65; refused(render(c), "65 points per path", "camera: points high");
  c = good; c.n_paths = 0; refused(render(c), "4 points per path", "camera: points without paths");
  c = good; c.fov = 0.0; refused(render(c), "fov 0", "camera: fov");
  c = good; c.fov = 3.0; refused(render(c), "fov 3", "camera: fov high");
  c = good; c.fov = __builtin_nan(""); refused(render(c), "fov nan", "camera: fov nan");
  c = good; c.mount_back = __builtin_inf(); refused(render(c), "mount_back inf", "camera: mount_back");
  c = good; c.cam_height = 0.0; refused(render(c), "cam_height 0", "camera: cam_height");
  c = good; c.near = 0.0; refused(render(c), "near 0", "camera: near");
  c = good; c.far = 0.05; refused(render(c), "far 0.05", "camera: far below near");
  c = good; c.far = __builtin_inf(); refused(render(c), "far inf", "camera: far");
  c = good; c.half_width = -1.0; refused(render(c), "half_width -1", "camera: half_width");
  c = good; c.mark = 2.0; refused(render(c), "mark 2", "camera: mark above half_width");
  c = good; c.mark = -0.1; refused(render(c), "mark -0.1", "camera: mark");
  c = good; c.line_half = 0.0; refused(render(c), "line_half 0", "camera: line_half");
  c = good; c.box_height = __builtin_nan(""); refused(render(c), "box_height nan", "camera: box_height");
  c = good; c.disc_height = 0.0; refused(render(c), "disc_height 0", "camera: disc_height");
  c = good; c.lamp_radius = 0.0; refused(render(c), "lamp_radius 0", "camera: lamp_radius");
  c = good; c.lamp_height = -4.0; refused(render(c), "lamp_height -4", "camera: lamp_height");
  c = good; c.lamp_setback = __builtin_nan(""); refused(render(c), "lamp_setback nan", "camera: lamp_setback");
  c = good; c.pole_radius = -0.1; refused(render(c), "pole_radius -0.1", "camera: pole_radius");
  c = good; c.mean[1] = __builtin_inff(); refused(render(c), "mean[1]", "camera: mean");
  c = good; c.stdv[2] = 0.f; refused(render(c), "std[2]", "camera: std");
  c = good; c.mark = 1.75; c.pole_radius = 0.0; c.n_boxes = c.n_discs = c.n_signals = 0; c.n_paths = 0; c.n_points = 0;      // edges in range:
  refused(camera_render(&c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, prims, frames.data(), nullptr, nullptr, nullptr,
                        nullptr),
          "null pose", "camera: the edges of the ranges and an empty world, then null pose");
#define RENDER(POSE, BOXES, DISCS, SIGNALS, PHASE, ROADS, LEN, HOLD, PRIMS, FRAMES, IMAGE, IDS, DEPTH) \
  camera_render(&good, POSE, BOXES, DISCS, SIGNALS, PHASE, ROADS, LEN, HOLD, PRIMS, FRAMES, IMAGE, IDS, DEPTH, nullptr)
  double* const P = pose.data(); double* const B = boxes.data(); double* const D = discs.data(); double* const G2 = signals.data();
  int32_t* const PH = phase.data(); double* const R = roads.data(); int32_t* const RL = road_len.data(); int32_t* const HO = hold.data();
  uint8_t* const FR = frames.data(); float* const IM = image.data(); int32_t* const ID = ids.data(); float* const DE = depth.data();
  refused(RENDER(P, nullptr, D, G2, PH, R, RL, HO, prims, FR, IM, ID, DE), "null boxes", "camera: null boxes");
  refused(RENDER(P, B, nullptr, G2, PH, R, RL, HO, prims, FR, IM, ID, DE), "null discs", "camera: null discs");
  refused(RENDER(P, B, D, nullptr, PH, R, RL, HO, prims, FR, IM, ID, DE), "null signals", "camera: null signals");
  refused(RENDER(P, B, D, G2, nullptr, R, RL, HO, prims, FR, IM, ID, DE), "null phase", "camera: null phase");
  refused(RENDER(P, B, D, G2, PH, nullptr, RL, HO, prims, FR, IM, ID, DE), "null roads", "camera: null roads");
  refused(RENDER(P, B, D, G2, PH, R, nullptr, HO, prims, FR, IM, ID, DE), "null road_len", "camera: null road_len");
  refused(RENDER(P, B, D, G2, PH, R, RL, HO, nullptr, FR, IM, ID, DE), "null prims", "camera: null prims");
  refused(RENDER(P, B, D, G2, PH, R, RL, HO, prims + 1, FR, IM, ID, DE), "16-byte aligned", "camera: prims alignment");
  refused(RENDER(P, B, D, G2, PH, R, RL, nullptr, prims, nullptr, nullptr, nullptr, nullptr), "no output", "camera: no output");
  refused(RENDER(P, B, D, G2, PH, R, RL, HO, reinterpret_cast<float*>(boxes.data()), FR, IM, ID, DE), "prims aliases boxes", "camera: prims on boxes");
  refused(RENDER(P, B, D, G2, PH, R, RL, HO, prims, reinterpret_cast<uint8_t*>(pose.data()), IM, ID, DE), "frames aliases pose", "camera: frames on pose");
  refused(RENDER(P, B, D, G2, PH, R, RL, HO, prims, FR, reinterpret_cast<float*>(discs.data()), ID, DE), "image aliases discs", "camera: image on discs");
  refused(RENDER(P, B, D, G2, PH, R, RL, HO, prims, FR, IM, PH, DE), "ids aliases phase", "camera: ids on phase");
  refused(RENDER(P, B, D, G2, PH, R, RL, HO, prims, FR, IM, HO, DE), "ids aliases hold", "camera: ids on hold");
  refused(RENDER(P, B, D, G2, PH, R, RL, HO, prims, FR, IM, ID, reinterpret_cast<float*>(signals.data())), "depth aliases signals",
          "camera: depth on signals");
  refused(RENDER(P, B, D, G2, PH, R, RL, HO, prims, FR, IM, ID, reinterpret_cast<float*>(roads.data() + 1)), "depth aliases roads",
          "camera: depth on roads");
  refused(RENDER(P, B, D, G2, PH, R, RL, HO, prims, FR, IM, RL, DE), "ids aliases road_len", "camera: ids on road_len");
  refused(RENDER(P, B, D, G2, PH, R, RL, HO, prims, reinterpret_cast<uint8_t*>(prims + 8), IM, ID, DE), "prims and frames alias each other",
          "camera: frames in prims");
  refused(RENDER(P, B, D, G2, PH, R, RL, HO, prims, FR, reinterpret_cast<float*>(FR + 4), ID, DE), "frames and image alias each other",
          "camera: image in frames");
  refused(RENDER(P, B, D, G2, PH, R, RL, HO, prims, FR, IM, reinterpret_cast<int32_t*>(IM + 2), DE), "image and ids alias each other",
          "camera: ids in image");
  refused(RENDER(P, B, D, G2, PH, R, RL, HO, prims, nullptr, nullptr, ID, reinterpret_cast<float*>(ID + 3)), "ids and depth alias each other",
          "camera: depth in ids");

  if (g_failed == 0) printf("camera host check: every refusal held\n");
  return g_failed == 0 ? 0 : 1;
}
