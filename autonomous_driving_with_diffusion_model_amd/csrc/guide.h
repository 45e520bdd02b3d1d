// "Cost guidance v1" (include/adx.h) on the device: the argument record of a guided launch and the ONE routine that evaluates a
// waypoint's cost.  The step kernels and guide_cost_kernel (sched.hip) and the guided select kernel (select.hip) all call it, so
// what a step steers by, what adx_guide_cost reports and what a selection scores are the same bits.
#pragma once
#include "adx_common.h"

namespace adx {

// Cost guidance v1: discs [scene_rows][M][5], planes [scene_rows][P][3]; row r of a launch reads scene r % scene_rows
struct GuideArgs {
  const float* discs;
  const float* planes;
  int scene_rows, M, P, iters;
  float lambda, cap;
};

// Cost guidance v1: the cost J of one waypoint (x, y) at index h (hf = (float)h) under one scene's M discs and P planes, its
// gradient and the number of active terms; the contract's operations in the contract's order, each rounded on its own
__device__ __forceinline__ void guide_grad(const float* discs, int M, const float* planes, int P, float hf, float x, float y,
                                           float& J, float& gx, float& gy, int& active) {
#pragma clang fp contract(off)
  J = 0.f; gx = 0.f; gy = 0.f; active = 0;
  for (int i = 0; i < M; ++i) {
    const float* q = discs + i * 5;
    const float r = q[4];
    if (!(r > 0.f)) continue;                  // an empty slot (a NaN radius too)
    const float hx = hf * q[2], hy = hf * q[3];
    const float ox = q[0] + hx, oy = q[1] + hy;
    const float dx = x - ox, dy = y - oy;
    const float xx = dx * dx, yy = dy * dy;
    const float d2 = xx + yy;
    const float rr = r * r;
    const float inv = 1.0f / rr;
    const float sd = d2 * inv;
    const float phi = 1.0f - sd;
    if (phi > 0.f) {
      const float pp = phi * phi;
      J = J + pp / 2.0f;
      const float k2 = 2.0f * phi;
      const float k = k2 * inv;
      const float kx = k * dx, ky = k * dy;
      gx = gx - kx;
      gy = gy - ky;
      ++active;
    }
  }
  for (int i = 0; i < P; ++i) {
    const float* q = planes + i * 3;
    const float nx = q[0], ny = q[1];
    const float ax = nx * x, ay = ny * y;
    const float psi = (ax + ay) - q[2];
    if (psi > 0.f) {
      const float pp = psi * psi;
      J = J + pp / 2.0f;
      const float px = psi * nx, py = psi * ny;
      gx = gx + px;
      gy = gy + py;
      ++active;
    }
  }
}

}  // namespace adx
