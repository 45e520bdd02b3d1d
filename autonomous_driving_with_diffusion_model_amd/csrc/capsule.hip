// "Capsules from boxes v1" (include/adx.h): the capsule slots of "cost guidance v5" from oriented boxes.  No reference counterpart.
//
// One thread per box, 256 threads per workgroup: a thread reads its box's eight floats and writes its seven, every operation
// rounded on its own.  At most 32 boxes per scene, so a launch is tiny -- what it buys is that a
// captured tick whose boxes change at every replay needs no host work.  The capsule is the box's inscribed stadium: the segment
// along the longer side, shortened by half the shorter side at each end, with half the shorter side (plus `inflate`) as radius.
#include "sched.h"

namespace adx {

namespace {

constexpr int kBoxThreads = 256;

struct BoxArgs {
  const float* boxes;
  float* out;
  int total;
  float inflate;
};

__global__ void __launch_bounds__(kBoxThreads) capsules_from_boxes_kernel(const BoxArgs a) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * kBoxThreads + threadIdx.x;
  if (i >= a.total) return;
  const float* q = a.boxes + (size_t)i * 8;
  const float cx = q[0], cy = q[1], vx = q[2], vy = q[3], ux = q[4], uy = q[5], length = q[6], width = q[7];
  float* o = a.out + (size_t)i * 7;
  if (!(length > 0.f && width > 0.f)) {      // not live (a NaN size too): an empty capsule
#pragma unroll
    for (int j = 0; j < 7; ++j) o[j] = 0.f;
    return;
  }
  const bool lon = length >= width;
  const float la = lon ? length : width, lb = lon ? width : length;
  const float ha = la / 2.0f, hb = lb / 2.0f;
  const float s = ha - hb;
  const float dx = lon ? ux : -uy, dy = lon ? uy : ux;
  const float ox = s * dx, oy = s * dy;
  o[0] = cx - ox; o[1] = cy - oy;
  o[2] = cx + ox; o[3] = cy + oy;
  o[4] = vx; o[5] = vy;
  o[6] = hb + a.inflate;
}

}  // namespace

int capsules_from_boxes(const float* boxes, float* out, int scenes, int n_boxes, float inflate, hipStream_t s) {
  ADX_REQUIRE(boxes != nullptr && out != nullptr, "capsules from boxes: null boxes or out");
  ADX_REQUIRE(n_boxes >= 1 && n_boxes <= ADX_CAPSULE_MAX, "capsules from boxes: n_boxes %d outside 1..%d", n_boxes, ADX_CAPSULE_MAX);
  ADX_REQUIRE(scenes >= 1 && scenes <= (1 << 20), "capsules from boxes: %d scenes, supported 1..%d", scenes, 1 << 20);
  ADX_REQUIRE(inflate >= 0.f && inflate < __builtin_inff(), "capsules from boxes: inflate %g is negative or not finite", (double)inflate);
  const size_t bn = (size_t)scenes * n_boxes * 8 * sizeof(float), on = (size_t)scenes * n_boxes * 7 * sizeof(float);
  const uintptr_t p = (uintptr_t)boxes, q = (uintptr_t)out;
  ADX_REQUIRE(!(p < q + on && q < p + bn), "capsules from boxes: out overlaps boxes");
  BoxArgs a;
  a.boxes = boxes; a.out = out; a.total = scenes * n_boxes; a.inflate = inflate;
  capsules_from_boxes_kernel<<<dim3(ceil_div(a.total, kBoxThreads)), dim3(kBoxThreads), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

}  // namespace adx
