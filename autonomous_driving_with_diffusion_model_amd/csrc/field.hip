// "Cost field from occupancy v1" (include/adx.h): a cost raster for "cost guidance v2" from a binary occupancy raster.  No reference
// counterpart.
//
// One workgroup per 8 x 32 output tile (256 threads: lane = x, so a wave's global reads and writes are two contiguous 128-byte
// rows), grid = (x tiles, y tiles, scenes): a 256 x 256 raster of 64 scenes is one launch of 8 x 32 x 64 workgroups.  The tile's
// occupancy and its halo of (ry, rx) nodes are staged ONCE in LDS as bytes (1 occupied, 0 free or outside the raster): at most
// 40 rows of 64 bytes = 2.5 KiB.  A search step then reads one byte per lane at consecutive addresses: the 32 lanes of a half
// wave touch 8 consecutive dwords, four lanes per dword (a broadcast), so no step has a bank conflict.  Every thread walks the
// whole (2 ry + 1) x (2 rx + 1) window: the trip count is the launch's, no lane diverges, and a minimum is exact in any order.
#include "sched.h"

namespace adx {

namespace {

constexpr int kTileX = 32, kTileY = 8, kMaxR = ADX_FIELD_MAX_RADIUS;
constexpr int kStageX = kTileX + 2 * kMaxR, kStageY = kTileY + 2 * kMaxR;      // 64 x 40

struct OccArgs {
  const float* occ;
  float* cells;
  int Gy, Gx, ry, rx;
  float dx, dy, inv_m2;
};

__global__ void __launch_bounds__(kTileX * kTileY) field_from_occupancy_kernel(const OccArgs a) {
#pragma clang fp contract(off)
  __shared__ uint8_t occ_s[kStageY * kStageX];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kTileX, y0 = blockIdx.y * kTileY;
  const size_t plane = (size_t)blockIdx.z * a.Gy * a.Gx;
  const float* occ = a.occ + plane;
  // stage rows [y0 - ry, y0 + kTileY + ry) x columns [x0 - rx, x0 + kTileX + rx); local (ly, lx) = node (y0 - ry + ly, x0 - rx + lx)
  const int sw = kTileX + 2 * a.rx, sh = kTileY + 2 * a.ry;      // <= kStageX, kStageY (the host checked rx, ry)
  for (int i = tid; i < sh * kStageX; i += kTileX * kTileY) {
    const int ly = i / kStageX, lx = i - ly * kStageX;
    const int y = y0 - a.ry + ly, x = x0 - a.rx + lx;
    uint8_t o = 0;
    if (lx < sw && y >= 0 && y < a.Gy && x >= 0 && x < a.Gx) o = occ[(size_t)y * a.Gx + x] > 0.5f ? 1 : 0;      // a NaN is free
    occ_s[i] = o;
  }
  __syncthreads();
  const int tx = tid & (kTileX - 1), ty = tid / kTileX;
  float best = __builtin_inff();
  for (int di = -a.ry; di <= a.ry; ++di) {
    const float sy = (float)di * a.dy;
    const float yy = sy * sy;
    const uint8_t* row = occ_s + (ty + a.ry + di) * kStageX + tx + a.rx;
    for (int dj = -a.rx; dj <= a.rx; ++dj) {
      const float sx = (float)dj * a.dx;
      const float xx = sx * sx;
      const float d2 = xx + yy;
      if (row[dj] != 0 && d2 < best) best = d2;
    }
  }
  const int x = x0 + tx, y = y0 + ty;
  if (x >= a.Gx || y >= a.Gy) return;
  float v = 0.f;
  if (best < __builtin_inff()) {
    const float sd = best * a.inv_m2;
    const float phi = 1.0f - sd;
    if (phi > 0.f) {
      const float pp = phi * phi;
      v = pp / 2.0f;
    }
  }
  a.cells[plane + (size_t)y * a.Gx + x] = v;
}

bool finite_pos(float v) { return v > 0.f && v < __builtin_inff(); }

}  // namespace

int field_from_occupancy(const float* occ, float* cells, int scenes, int gy, int gx, float dx, float dy, float inv_m2, int ry, int rx,
                         hipStream_t s) {
  ADX_REQUIRE(occ != nullptr && cells != nullptr, "cost field from occupancy: null occ or cells");
  ADX_REQUIRE(scenes >= 1 && scenes <= 65535, "cost field from occupancy: %d scenes, supported 1..65535", scenes);
  ADX_REQUIRE(gx >= ADX_FIELD_MIN_NODES && gx <= ADX_FIELD_MAX_NODES && gy >= ADX_FIELD_MIN_NODES && gy <= ADX_FIELD_MAX_NODES,
              "cost field from occupancy: raster of %d x %d nodes (gy x gx), supported %d..%d each", gy, gx, ADX_FIELD_MIN_NODES,
              ADX_FIELD_MAX_NODES);
  ADX_REQUIRE(rx >= 0 && rx <= kMaxR && ry >= 0 && ry <= kMaxR, "cost field from occupancy: window radii (ry %d, rx %d) outside 0..%d",
              ry, rx, kMaxR);
  ADX_REQUIRE(finite_pos(dx) && finite_pos(dy), "cost field from occupancy: cell size (%g, %g) must be finite and > 0", (double)dx,
              (double)dy);
  ADX_REQUIRE(finite_pos(inv_m2), "cost field from occupancy: inv_m2 %g must be finite and > 0", (double)inv_m2);
  const size_t n = (size_t)scenes * gy * gx * sizeof(float);
  const uintptr_t p = (uintptr_t)occ, q = (uintptr_t)cells;
  ADX_REQUIRE(!(p < q + n && q < p + n), "cost field from occupancy: cells overlaps occ");
  OccArgs a;
  a.occ = occ; a.cells = cells; a.Gy = gy; a.Gx = gx; a.ry = ry; a.rx = rx; a.dx = dx; a.dy = dy; a.inv_m2 = inv_m2;
  field_from_occupancy_kernel<<<dim3(ceil_div(gx, kTileX), ceil_div(gy, kTileY), scenes), dim3(kTileX * kTileY), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

}  // namespace adx
