// "Cost guidance v1" and "cost guidance v2" (include/adx.h) on the device: the argument record of a guided launch (GuideArgs), the
// view of one scene of it that a row resolves once (SceneGuide, scene_guide) and the ONE routine that evaluates a waypoint's cost
// under that view (guide_grad).  The step kernels and guide_cost_kernel (sched.hip), the guided select kernel (select.hip) and the
// stop-short kernel (fallback.hip) all call it, so what a step steers by, what adx_guide_cost reports, what a selection scores and
// what the fallback stops for are the same bits.
// "Cost guidance v4" adds the route corridor to that routine, after the field term: a per-scene polyline and a half-width.
// "Cost guidance v5" adds moving capsules to that routine, after the route term: per scene up to 32 segments with a radius.
// "Cost guidance v3" adds motion_grad beside it: a waypoint's share of the terms that couple it to its neighbours, for the row-wise
// step kernels, guide_cost_kernel<true> and traj_select_kernel<true, true>.
#pragma once
#include "adx_common.h"

namespace adx {

// Cost guidance v2: cells [scene_rows][Gy][Gx], node [0][0] at (x_min, y_min); row r of a launch reads scene r % scene_rows.
// cells == nullptr: no field, and nothing else of the record is read
struct FieldArgs {
  const float* cells;
  int scene_rows, Gx, Gy;
  float x_min, y_min, inv_dx, inv_dy, weight;
};

// Cost guidance v4: points [scene_rows][R][2], half_width [scene_rows]; row r of a launch reads scene r % scene_rows.
// points == nullptr: no route, and nothing else of the record is read
struct RouteArgs {
  const float* points;
  const float* half_width;
  int scene_rows, R;
  float weight;
};

// Cost guidance v5: slots [scene_rows][C][7] = (ax, ay, bx, by, vx, vy, r); row r of a launch reads scene r % scene_rows.
// slots == nullptr: no capsules, and nothing else of the record is read
struct CapsuleArgs {
  const float* slots;
  int scene_rows, C;
  float weight;
};

// Cost guidance v1: discs [scene_rows][M][5], planes [scene_rows][P][3]; row r of a launch reads scene r % scene_rows
struct GuideArgs {
  const float* discs;
  const float* planes;
  int scene_rows, M, P, iters;
  float lambda, cap;
  FieldArgs field;      // cost guidance v2
  RouteArgs route;      // cost guidance v4
  CapsuleArgs capsule;  // cost guidance v5
};

// One scene of a guided launch: what guide_grad reads, resolved ONCE per row by scene_guide.  A pointer is null where its term is
// not evaluated, which is the same in every thread of a launch.  A value that lives in registers: after inlining nothing of it
// is left but the operands guide_grad uses.
struct SceneGuide {
  const float* discs;      // [M][5]
  const float* planes;     // [P][3]
  const float* cells;      // the scene's raster; null without a field
  const float* pts;        // the scene's polyline [R][2]; null without a route or at weight 0
  const float* caps;       // the scene's slots [C][7]; null without capsules or at weight 0
  int M, P, R, C;
  float W2, rw, cw;        // the route's squared half-width (one rounded product) and weight; the capsules' weight
  FieldArgs field;         // the field's geometry and weight
};

// The polyline of row `row`'s scene, or nullptr without a route or at weight 0, where the term is not evaluated
__device__ __forceinline__ const float* route_points(const RouteArgs& r, int row) {
  return r.points == nullptr || r.weight == 0.f ? nullptr : r.points + (size_t)(row % r.scene_rows) * r.R * 2;
}

// The view of row `row`'s scene.  The route's and the capsules' arrays are read from global memory as they lie: a scene's points
// are at most 256 bytes and its capsules at most 896 that every lane of the scene reads at the same addresses.
// What the view holds does not depend on the order its pointers are formed in; what a kernel's prologue costs does, by a per cent
// or two (profiles/README.md, "One guide bundle").  So the two things a call site may want to place are explicit, and there are no
// others: `scene`, which is row % g.scene_rows, is a parameter so that guide_x0 can form it ahead of its partner element's loads,
// where the division costs nothing; kRouteFirst forms the route's pointer ahead of the discs' and planes', which is the order the
// wave-per-row kernels (guide_cost_kernel, stop_short_kernel) were measured with.  Everyone else calls the plain two-argument form.
template <bool kRouteFirst = false>
__device__ __forceinline__ SceneGuide scene_guide(const GuideArgs& g, int row, int scene) {
#pragma clang fp contract(off)
  SceneGuide v;
  const RouteArgs& r = g.route;
  if constexpr (kRouteFirst) v.pts = route_points(r, row);
  v.discs = g.discs + (size_t)scene * g.M * 5;
  v.planes = g.planes + (size_t)scene * g.P * 3;
  const FieldArgs& f = g.field;
  v.cells = f.cells == nullptr ? nullptr : f.cells + (size_t)(row % f.scene_rows) * f.Gy * f.Gx;
  if constexpr (!kRouteFirst) v.pts = route_points(r, row);
  v.W2 = 0.f;
  if (v.pts != nullptr) {
    const float w = r.half_width[row % r.scene_rows];
    v.W2 = w * w;
  }
  const CapsuleArgs& c = g.capsule;
  v.caps = c.slots == nullptr || c.weight == 0.f ? nullptr : c.slots + (size_t)(row % c.scene_rows) * c.C * 7;
  v.M = g.M; v.P = g.P; v.R = r.R; v.C = c.C;
  v.rw = r.weight; v.cw = c.weight;
  v.field = f;
  return v;
}

template <bool kRouteFirst = false>
__device__ __forceinline__ SceneGuide scene_guide(const GuideArgs& g, int row) {
  return scene_guide<kRouteFirst>(g, row, row % g.scene_rows);
}

// Cost guidance v1 / v2 / v4 / v5: the cost J of one waypoint (x, y) at index h (hf = (float)h) under its scene `s`: the M discs and
// P planes, then the field where s.cells is not null, then the route (the nearest of the R - 1 segments against W2 at weight rw)
// where s.pts is not null, then the C capsule slots at weight cw (each v1's disc potential around the nearest point of its moved
// segment) where s.caps is not null; its gradient and the number of active terms.  The contracts' operations in the contracts'
// order, each rounded on its own; an absent term adds nothing, so without it the accumulation is the earlier version's, bit for
// bit.  A new term adds a field to SceneGuide and a block here, and touches no call site.
__device__ __forceinline__ void guide_grad(const SceneGuide& s, float hf, float x, float y, float& J, float& gx, float& gy, int& active) {
#pragma clang fp contract(off)
  J = 0.f; gx = 0.f; gy = 0.f; active = 0;
  for (int i = 0; i < s.M; ++i) {
    const float* q = s.discs + i * 5;
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
  for (int i = 0; i < s.P; ++i) {
    const float* q = s.planes + i * 3;
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
  if (s.cells != nullptr) {      // the field term: the bilinear interpolant of the cell the waypoint lies in, and its exact gradient
    const FieldArgs& f = s.field;
    const float ux = x - f.x_min, vy = y - f.y_min;
    const float u = ux * f.inv_dx, v = vy * f.inv_dy;
    const int Gx = f.Gx, Gy = f.Gy;
    if (u >= 0.f && u <= (float)(Gx - 1) && v >= 0.f && v <= (float)(Gy - 1)) {      // a NaN is outside
      const int ju = (int)u, iv = (int)v;
      const int j = ju < Gx - 2 ? ju : Gx - 2, i = iv < Gy - 2 ? iv : Gy - 2;       // 0 <= j <= Gx - 2, 0 <= i <= Gy - 2
      const float fu = u - (float)j, fv = v - (float)i;
      const float* c = s.cells + (size_t)i * Gx + j;
      const float c00 = c[0], c01 = c[1], c10 = c[Gx], c11 = c[Gx + 1];
      const float a = c01 - c00, b = c11 - c10;
      const float ta = fu * a, tb = fu * b;
      const float top = c00 + ta, bot = c10 + tb;
      const float dv = bot - top;
      const float tv = fv * dv;
      const float C = top + tv;
      if (C > 0.f) {
        const float ba = b - a;
        const float tu = fv * ba;
        const float du = a + tu;
        const float wc = f.weight * C;
        J = J + wc;
        const float wu = f.weight * du, wv = f.weight * dv;
        const float sx = wu * f.inv_dx, sy = wv * f.inv_dy;
        gx = gx + sx;
        gy = gy + sy;
        ++active;
      }
    }
  }
  if (s.pts != nullptr) {      // the route term: the squared distance to the nearest segment over W2; no square root
    const float* pts = s.pts;
    float best = __builtin_inff(), qx = 0.f, qy = 0.f;
    float ax = pts[0], ay = pts[1];
    for (int i = 1; i < s.R; ++i) {
      const float bx = pts[2 * i], by = pts[2 * i + 1];
      const float ex = bx - ax, ey = by - ay;
      const float ux = x - ax, uy = y - ay;
      const float exx = ex * ex, eyy = ey * ey;
      const float ee = exx + eyy;
      const float uxe = ux * ex, uye = uy * ey;
      const float ue = uxe + uye;
      float t = ee > 0.f ? ue / ee : 0.f;       // a degenerate segment is its first point
      t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);      // a NaN passes through
      const float tx = t * ex, ty = t * ey;
      const float rx = ux - tx, ry = uy - ty;
      const float rxx = rx * rx, ryy = ry * ry;
      const float d2 = rxx + ryy;
      if (d2 < best) { best = d2; qx = rx; qy = ry; }      // strict: the first of equals wins; a NaN never wins
      ax = bx; ay = by;
    }
    const float phi = best - s.W2;
    if (best < __builtin_inff() && phi > 0.f) {
      const float pp = phi * phi;
      const float wp = s.rw * pp;
      J = J + wp / 2.0f;
      const float p2 = 2.0f * phi;
      const float k = s.rw * p2;
      const float kx = k * qx, ky = k * qy;
      gx = gx + kx;
      gy = gy + ky;
      ++active;
    }
  }
  if (s.caps != nullptr) {      // the capsule term: v1's disc potential around the nearest point of each moved segment; no square root
    for (int i = 0; i < s.C; ++i) {
      const float* q = s.caps + i * 7;
      const float r = q[6];
      if (!(r > 0.f)) continue;                  // an empty slot (a NaN radius too)
      const float ax = q[0], ay = q[1];
      const float hx = hf * q[4], hy = hf * q[5];
      const float px = ax + hx, py = ay + hy;
      const float ex = q[2] - ax, ey = q[3] - ay;      // from the unmoved ends: both move alike
      const float ux = x - px, uy = y - py;
      const float exx = ex * ex, eyy = ey * ey;
      const float ee = exx + eyy;
      const float uxe = ux * ex, uye = uy * ey;
      const float ue = uxe + uye;
      float t = ee > 0.f ? ue / ee : 0.f;       // a == b: a disc around a
      t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);      // a NaN passes through
      const float tx = t * ex, ty = t * ey;
      const float rx = ux - tx, ry = uy - ty;
      const float rxx = rx * rx, ryy = ry * ry;
      const float d2 = rxx + ryy;
      const float rr = r * r;
      const float inv = 1.0f / rr;
      const float sd = d2 * inv;
      const float phi = 1.0f - sd;
      if (phi > 0.f) {
        const float pp = phi * phi;
        const float wp = s.cw * pp;
        J = J + wp / 2.0f;
        const float p2 = 2.0f * phi;
        const float pk = p2 * inv;
        const float k = s.cw * pk;
        const float kx = k * rx, ky = k * ry;
        gx = gx - kx;
        gy = gy - ky;
        ++active;
      }
    }
  }
}

// Cost guidance v3: limits [scene_rows][2] = (s_max, a_max); row r of a launch reads scene r % scene_rows.
// limits == nullptr: no motion limits, and nothing else of the record is read
struct MotionArgs {
  const float* limits;
  int scene_rows;
  float w_speed, w_accel;
};

// (S2, A2) of row `row`'s scene: the squares of its limits, each one rounded product
__device__ __forceinline__ void motion_limits(const MotionArgs& m, int row, float& S2, float& A2) {
#pragma clang fp contract(off)
  const float* q = m.limits + (size_t)(row % m.scene_rows) * 2;
  const float s = q[0], a = q[1];
  S2 = s * s;
  A2 = a * a;
}

// The segment from a to b against S2: e = b - a and k = w * (2 * phi) where phi = |e|^2 - S2 > 0, else inactive (a NaN too)
__device__ __forceinline__ bool motion_segment(float ax, float ay, float bx, float by, float S2, float w, float& ex, float& ey, float& phi,
                                               float& k) {
#pragma clang fp contract(off)
  ex = bx - ax; ey = by - ay;
  const float xx = ex * ex, yy = ey * ey;
  const float s2 = xx + yy;
  phi = s2 - S2;
  if (!(phi > 0.f)) return false;
  const float p2 = 2.0f * phi;
  k = w * p2;
  return true;
}

// The second difference at b between a and c against A2: c = (c - b) - (b - a) and q = w * (2 * psi) where psi = |c|^2 - A2 > 0
__device__ __forceinline__ bool motion_curvature(float ax, float ay, float bx, float by, float cx_, float cy_, float A2, float w, float& cx,
                                                 float& cy, float& psi, float& q) {
#pragma clang fp contract(off)
  const float fx = cx_ - bx, fy = cy_ - by;
  const float bx_ = bx - ax, by_ = by - ay;
  cx = fx - bx_; cy = fy - by_;
  const float xx = cx * cx, yy = cy * cy;
  const float a2 = xx + yy;
  psi = a2 - A2;
  if (!(psi > 0.f)) return false;
  const float p2 = 2.0f * psi;
  q = w * p2;
  return true;
}

// Cost guidance v3: waypoint h's share of the segment and curvature terms of a row of H waypoints, added to J, gx, gy and active
// AFTER guide_grad filled them.  (x[j], y[j]) = p_{h-2+j}, j = 0..4; a point outside 0..H-1 is never read into a result (its term
// does not exist).  The contract's operations in the contract's order, each rounded on its own; an inactive or absent term adds
// nothing, not even a zero.  The neighbours are the caller's to bring: a shuffle in the row-wise kernels, LDS in the selection.
__device__ __forceinline__ void motion_grad(const float* x, const float* y, int h, int H, float S2, float A2, float w_speed, float w_accel,
                                            float& J, float& gx, float& gy, int& active) {
#pragma clang fp contract(off)
  float ex, ey, phi, k, cx, cy, psi, q;
  const bool anchor = h == 0;      // the ego's present pose takes no motion gradient
  if (w_speed != 0.f) {
    if (h >= 1 && motion_segment(x[1], y[1], x[2], y[2], S2, w_speed, ex, ey, phi, k)) {        // segment h - 1: p_h is its far end
      const float pp = phi * phi;
      const float wp = w_speed * pp;
      J = J + wp / 2.0f;
      ++active;
      const float kx = k * ex, ky = k * ey;
      gx = gx + kx;
      gy = gy + ky;
    }
    if (!anchor && h <= H - 2 && motion_segment(x[2], y[2], x[3], y[3], S2, w_speed, ex, ey, phi, k)) {      // segment h: its near end
      const float kx = k * ex, ky = k * ey;
      gx = gx - kx;
      gy = gy - ky;
    }
  }
  if (w_accel != 0.f) {
    if (h >= 2 && motion_curvature(x[0], y[0], x[1], y[1], x[2], y[2], A2, w_accel, cx, cy, psi, q)) {      // curvature h - 1
      const float qx = q * cx, qy = q * cy;
      gx = gx + qx;
      gy = gy + qy;
    }
    if (h >= 1 && h <= H - 2 && motion_curvature(x[1], y[1], x[2], y[2], x[3], y[3], A2, w_accel, cx, cy, psi, q)) {      // curvature h
      const float pp = psi * psi;
      const float wp = w_accel * pp;
      J = J + wp / 2.0f;
      ++active;
      const float q2 = 2.0f * q;
      const float qx = q2 * cx, qy = q2 * cy;
      gx = gx - qx;
      gy = gy - qy;
    }
    if (!anchor && h <= H - 3 && motion_curvature(x[2], y[2], x[3], y[3], x[4], y[4], A2, w_accel, cx, cy, psi, q)) {      // curvature h + 1
      const float qx = q * cx, qy = q * cy;
      gx = gx + qx;
      gy = gy + qy;
    }
  }
}

}  // namespace adx
