// The front camera of the closed loop (include/adx.h: "camera v1"): an analytic ray caster over the primitives the loop already
// holds -- the ground with its roads and stop lines, the world's boxes and discs, the lamps and poles of its signals -- that writes
// the frame the encoder reads, one C call per tick.
//
//   camera_stage_kernel   one workgroup of one wave per scene, like drive.hip and signals.hip: lane j owns box j, disc j and signal
//                         j, then the lanes stride over the road segments.  fp64, no contraction, ego frame v1's rotate with the
//                         same cos and sin; every word of the primitive table is rounded to fp32 once.  The table also carries what
//                         depends on the primitive and the eye alone (the eye in a box's axes, a cylinder's r^2, a
//                         segment's 1 / |e|^2) and a conservative pixel rectangle per object.
//   camera_render_kernel  throughput-bound: one workgroup of 256 threads per 64 x 16 tile of one scene, a wave per row of 64
//                         columns, four rows per thread.  Thread i tests object i's rectangle against the tile; a ballot and the
//                         population count of the bits below a lane compact the survivors into an LDS list in index order.  The
//                         ground records are copied to LDS only by tiles that reach below the horizon.  Every lane of a wave walks
//                         the same record, so the LDS reads are broadcasts and the kind switch is uniform.  fp32 only, + - * / sqrt
//                         and comparisons, each rounded on its own: a NumPy float32 restatement on the same table decides alike.
// No atomics, no traffic between workgroups, no scalar-memory tricks and no inline assembly.
#include "sched.h"

#pragma clang fp contract(off)

namespace adx {

namespace {

constexpr int kCamMaxScenes = 65535, kCamMaxSlots = 64, kCamMaxPaths = 8, kCamMaxPoints = 64;
constexpr int kHdrWords = 16, kObjWords = 16, kGndWords = 8;
constexpr int kTileW = 64, kTileH = 16, kRows = 4;      // 256 threads: wave w owns rows w, w + 4, w + 8, w + 12 of the tile
constexpr int kMaxObj = 4 * kCamMaxSlots, kMaxGnd = kCamMaxSlots + kCamMaxPaths * (kCamMaxPoints - 1);
constexpr int kPalWords = 28;      // 20 palette rows and 5 shades, padded
static_assert((kMaxObj * kObjWords + kMaxGnd * kGndWords + kPalWords + 4) * 4 <= 64 * 1024, "camera v1: the render workgroup's LDS");
constexpr int kSky = 0, kGround = 1, kRoad = 2, kMark = 3, kLine = 4, kBox = 5, kDisc = 6, kLamp = 7, kPole = 8;
constexpr int kWhole0 = -1, kWhole1 = 1 << 20;
constexpr double kHalfPi = 1.57079632679489661923;
constexpr double kCullY = 0.05;      // a corner nearer the eye's plane than this cannot be projected safely: the whole image
constexpr double kCullRel = 1.0 / 1048576.0;      // 2^-20 of a corner's coordinates: far above the fp32 rounding of the table

struct CamArgs {
  const double *pose, *boxes, *discs, *signals, *roads;
  const int32_t *phase, *road_len, *hold;
  float* prims;
  uint8_t* frames;
  float* image;
  int32_t* ids;
  float* depth;
  int W, H, NB, ND, NS, Q, G, n_obj, n_gnd, scene_words;
  double k64, mount_back, height, box_height, disc_height, lamp_radius, lamp_height, lamp_setback, pole_radius;
  float k, hgt, near, far, r_in2, r_out2, line2;
  float mean[3], stdv[3];
  uint8_t palette[ADX_CAMERA_PALETTE][3];
  uint8_t shade[5];
};

// ---------------------------------------------------------------- stage ----------------------------------------------------------------

// Every word of the table goes out as one 32-bit store per lane (volatile keeps the compiler from merging neighbours): a wide store
// whose data registers the next VALU instruction overwrites is the pattern tools/check_store_hazard.py exists to catch, and narrow
// stores cannot form it (vehicle.hip's reason).  The launch is latency-bound, so the width of its stores costs nothing.

struct Cull {
  double u0 = 1e30, u1 = -1e30, v0 = 1e30, v1 = -1e30;
  bool nan = false, low = false;
  int front = 0;
};

__device__ void cull_add(Cull& c, double x, double y, double z, double k, int W, int H) {
  if (x != x || y != y || z != z) {
    c.nan = true;
    return;
  }
  const double err = kCullRel * (((fabs(x) + fabs(y)) + fabs(z)) + 1.0);
  if (y + err > 0.0) c.front += 1;
  if (y < kCullY) {
    c.low = true;
    return;
  }
  const double yk = y * k;
  const double u = x / yk + (0.5 * W - 0.5), v = (0.5 * H - 0.5) - z / yk;
  const double du = 1.0 + err * (1.0 + fabs(x) / y) / yk, dv = 1.0 + err * (1.0 + fabs(z) / y) / yk;
  c.u0 = fmin(c.u0, u - du);
  c.u1 = fmax(c.u1, u + du);
  c.v0 = fmin(c.v0, v - dv);
  c.v1 = fmax(c.v1, v + dv);
}

__device__ int cull_int(double v) { return (int)fmin(fmax(v, -1048576.0), 1048576.0); }

__device__ void cull_store(const Cull& c, volatile float* rec) {
  volatile int32_t* o = reinterpret_cast<volatile int32_t*>(rec);
  if (c.nan || (c.front > 0 && c.low)) {
    o[1] = kWhole0; o[2] = kWhole1; o[3] = kWhole0; o[4] = kWhole1;
  } else if (c.front == 0) {      // wholly behind the eye's plane: no t > near reaches it
    o[1] = 1; o[2] = 0; o[3] = 1; o[4] = 0;
  } else {
    o[1] = cull_int(floor(c.u0)); o[2] = cull_int(ceil(c.u1)); o[3] = cull_int(floor(c.v0)); o[4] = cull_int(ceil(c.v1));
  }
}

__device__ void empty_record(volatile float* rec, int words) {
  for (int w = 0; w < words; ++w) rec[w] = 0.f;
}

struct Frame {
  double px, py, c, s, mount_back;
  // ego frame v1's rotate, metres: the ego vector of a world vector
  __device__ void rotate(double dx, double dy, double& x, double& y) const {
    const double a0 = c * dx, a1 = s * dy;
    const double r0 = a0 + a1;
    const double b0 = s * dx, b1 = c * dy;
    const double r1 = -b0 + b1;
    x = r1;
    y = -r0;
  }
  // a world point in the camera frame (the eye at the origin; z is the caller's)
  __device__ void point(double X, double Y, double& x, double& y) const {
    double ex, ey;
    rotate(X - px, Y - py, ex, ey);
    x = ex;
    y = ey - mount_back;
  }
};

// a vertical cylinder of radius r over (cx, cy) from zlo to zhi, camera frame
__device__ void stage_cylinder(volatile float* rec, int id, double cx, double cy, double r, double zlo, double zhi, const CamArgs& a) {
  const double c0 = cx * cx, c1 = cy * cy;
  const double r2 = r * r;
  const double cc = (c0 + c1) - r2;
  const bool inside = cc <= 0.0 && zlo <= 0.0 && zhi >= 0.0;
  if (!(r > 0.0) || !(zhi > zlo) || inside || cc != cc) {
    empty_record(rec, kObjWords);
    return;
  }
  reinterpret_cast<volatile int32_t*>(rec)[0] = id;
  rec[5] = (float)cx; rec[6] = (float)cy; rec[7] = (float)r2; rec[8] = (float)zlo; rec[9] = (float)zhi;
  for (int w = 10; w < kObjWords; ++w) rec[w] = 0.f;
  Cull c;
  for (int i = 0; i < 8; ++i)
    cull_add(c, (i & 1) ? cx + r : cx - r, (i & 2) ? cy + r : cy - r, (i & 4) ? zhi : zlo, a.k64, a.W, a.H);
  cull_store(c, rec);
}

__global__ void __launch_bounds__(64) camera_stage_kernel(const CamArgs a) {
  const int s = blockIdx.x, lane = threadIdx.x;
  if (a.hold != nullptr && a.hold[s] != 0) return;
  volatile float* tab = a.prims + (size_t)s * a.scene_words;
  const double c2 = a.pose[(size_t)s * 3 + 2];
  const double th = (c2 != c2 ? 0.0 : c2) + kHalfPi;      // "frame" of ego frame v1: the same two library calls
  Frame f;
  f.px = a.pose[(size_t)s * 3 + 0];
  f.py = a.pose[(size_t)s * 3 + 1];
  f.c = cos(th);
  f.s = sin(th);
  f.mount_back = a.mount_back;
  const double zg = -a.height;      // the ground in the camera frame
  if (lane < kHdrWords) reinterpret_cast<volatile int32_t*>(tab)[lane] = lane == 0 ? 1 : (lane == 1 ? a.n_obj : (lane == 2 ? a.n_gnd : 0));
  volatile float* obj = tab + kHdrWords;
  volatile float* gnd = obj + (size_t)a.n_obj * kObjWords;

  // ---- box `lane` ----
  if (lane < a.NB) {
    const double* g = a.boxes + ((size_t)s * a.NB + lane) * 7;
    volatile float* rec = obj + (size_t)lane * kObjWords;
    const double yaw = g[4], hl = g[5] / 2.0, hw = g[6] / 2.0;
    double bx, by, ax, ay;
    f.point(g[0], g[1], bx, by);
    f.rotate(cos(yaw), sin(yaw), ax, ay);
    const double m0 = bx * ax, m1 = by * ay;
    const double el = -(m0 + m1);      // the eye in the box's axes: along the length,
    const double m2 = bx * ay, m3 = by * ax;
    const double ew = m2 - m3;         // along the width axis (-ay, ax)
    const double zhi = zg + a.box_height;
    const bool inside = el >= -hl && el <= hl && ew >= -hw && ew <= hw && zg <= 0.0 && zhi >= 0.0;
    if (!(hl > 0.0) || !(hw > 0.0) || inside || el != el || ew != ew) {
      empty_record(rec, kObjWords);
    } else {
      reinterpret_cast<volatile int32_t*>(rec)[0] = kBox << 8 | lane;
      rec[5] = (float)ax; rec[6] = (float)ay;
      rec[7] = (float)(-hl - el); rec[8] = (float)(hl - el); rec[9] = (float)(-hw - ew); rec[10] = (float)(hw - ew);
      rec[11] = (float)zg; rec[12] = (float)zhi;
      rec[13] = rec[14] = rec[15] = 0.f;
      Cull c;
      for (int i = 0; i < 8; ++i) {
        const double sl = (i & 1) ? hl : -hl, sw = (i & 2) ? hw : -hw;
        cull_add(c, (bx + sl * ax) - sw * ay, (by + sl * ay) + sw * ax, (i & 4) ? zhi : zg, a.k64, a.W, a.H);
      }
      cull_store(c, rec);
    }
  }
  // ---- disc `lane` ----
  if (lane < a.ND) {
    const double* g = a.discs + ((size_t)s * a.ND + lane) * 5;
    double cx, cy;
    f.point(g[0], g[1], cx, cy);
    stage_cylinder(obj + (size_t)(a.NB + lane) * kObjWords, kDisc << 8 | lane, cx, cy, g[4], zg, zg + a.disc_height, a);
  }
  // ---- signal `lane`: its lamp, its pole, its stop line ----
  if (lane < a.NS) {
    const double* g = a.signals + ((size_t)s * a.NS + lane) * 10;
    const int ph = a.phase[(size_t)s * a.NS + lane];
    volatile float* lamp = obj + (size_t)(a.NB + a.ND + lane) * kObjWords;
    volatile float* pole = obj + (size_t)(a.NB + a.ND + a.NS + lane) * kObjWords;
    volatile float* line = gnd + (size_t)lane * kGndWords;
    const double ddx = g[2] - g[0], ddy = g[3] - g[1];
    const double dxx = ddx * ddx, dyy = ddy * ddy;
    const double L = sqrt(dxx + dyy);
    if (ph < 1 || ph > 4 || !(L > 0.0)) {
      empty_record(lamp, kObjWords);
      empty_record(pole, kObjWords);
      empty_record(line, kGndWords);
    } else {
      // signals v1's t and n; the lamp stands beyond the line, on the far side of the junction
      const double tx = ddx / L, ty = ddy / L;
      const double nx = -ty, ny = tx;
      const double mx = g[0] + 0.5 * ddx, my = g[1] + 0.5 * ddy;
      const double wx = mx + a.lamp_setback * nx, wy = my + a.lamp_setback * ny;
      double lx, ly;
      f.point(wx, wy, lx, ly);
      const double lz = zg + a.lamp_height, R = a.lamp_radius;
      const double q0 = lx * lx, q1 = ly * ly, q2 = lz * lz;
      const double cc = ((q0 + q1) + q2) - R * R;
      if (!(cc > 0.0)) {      // the eye inside the lamp (or a NaN)
        empty_record(lamp, kObjWords);
      } else {
        volatile int32_t* li = reinterpret_cast<volatile int32_t*>(lamp);
        li[0] = kLamp << 8 | lane;
        lamp[5] = (float)lx; lamp[6] = (float)ly; lamp[7] = (float)lz; lamp[8] = (float)(R * R);
        li[9] = ph;
        for (int w = 10; w < kObjWords; ++w) lamp[w] = 0.f;
        Cull c;
        for (int i = 0; i < 8; ++i) cull_add(c, (i & 1) ? lx + R : lx - R, (i & 2) ? ly + R : ly - R, (i & 4) ? lz + R : lz - R, a.k64, a.W, a.H);
        cull_store(c, lamp);
      }
      stage_cylinder(pole, kPole << 8 | lane, lx, ly, a.pole_radius, zg, lz, a);
      double ax, ay, bx, by;
      f.point(g[0], g[1], ax, ay);
      f.point(g[2], g[3], bx, by);
      const double ex = bx - ax, ey = by - ay;
      const double e0 = ex * ex, e1 = ey * ey;
      const double e2 = e0 + e1;
      line[0] = (float)ax; line[1] = (float)ay; line[2] = (float)ex; line[3] = (float)ey;
      line[4] = e2 > 0.0 ? (float)(1.0 / e2) : 0.f;
      reinterpret_cast<volatile int32_t*>(line)[5] = e2 == e2 ? 1 : 0;
      line[6] = line[7] = 0.f;
    }
  }
  // ---- the road segments ----
  const int per = a.G - 1;
  for (int i = lane; i < a.Q * per; i += 64) {
    const int q = i / per, g0 = i - q * per;
    volatile float* seg = gnd + (size_t)(a.NS + i) * kGndWords;
    int len = a.road_len[(size_t)s * a.Q + q];
    len = len < 0 ? 0 : (len > a.G ? a.G : len);
    if (g0 + 1 >= len) {
      empty_record(seg, kGndWords);
      continue;
    }
    const double* p = a.roads + (((size_t)s * a.Q + q) * a.G + g0) * 2;
    double ax, ay, bx, by;
    f.point(p[0], p[1], ax, ay);
    f.point(p[2], p[3], bx, by);
    const double ex = bx - ax, ey = by - ay;
    const double e0 = ex * ex, e1 = ey * ey;
    const double e2 = e0 + e1;
    seg[0] = (float)ax; seg[1] = (float)ay; seg[2] = (float)ex; seg[3] = (float)ey;
    seg[4] = e2 > 0.0 ? (float)(1.0 / e2) : 0.f;
    reinterpret_cast<volatile int32_t*>(seg)[5] = e2 == e2 ? 1 : 0;      // a NaN point: no segment
    seg[6] = seg[7] = 0.f;
  }
}

// ---------------------------------------------------------------- render ----------------------------------------------------------------

struct Best {
  float t;
  int id, aux;
};

// the hit rule: t > near, the nearest wins, an exact tie goes to the lower class << 8 | slot
__device__ __forceinline__ void consider(Best& b, float t, int id, int aux, float near) {
  if (t > near && (t < b.t || (t == b.t && (id & 0xffff) < (b.id & 0xffff)))) {
    b.t = t;
    b.id = id;
    b.aux = aux;
  }
}

__device__ __forceinline__ void slab(float d, float n0, float n1, int axis, float& tn, float& tf, int& face, bool& ok) {
  if (d == 0.f) {      // parallel to the slab: inside it or a miss, never a division
    if (!(n0 <= 0.f && n1 >= 0.f)) ok = false;
    return;
  }
  const float t1 = n0 / d, t2 = n1 / d;
  const bool up = d > 0.f;
  const float lo = up ? t1 : t2, hi = up ? t2 : t1;
  if (lo > tn) {      // strictly: on a tie the lower axis keeps the face
    tn = lo;
    face = axis == 2 ? 4 : 2 * axis + (up ? 0 : 1);
  }
  if (hi < tf) tf = hi;
}

__device__ __forceinline__ void hit_cylinder(Best& b, const float* r, int id, float dx, float dz, float A2, float near) {
  const float cx = r[5], cy = r[6], r2 = r[7], zlo = r[8], zhi = r[9];
  const float B = dx * cx + cy;
  const float cr = dx * cy - cx;      // the ray's direction x the centre: |.|^2 / A2 is the squared distance of the axis
  const float q = A2 * r2;
  const float disc = q - cr * cr;
  if (disc >= 0.f) {
    const float sq = __builtin_sqrtf(disc);
    const float ts = (B - sq) / A2;
    const float zs = ts * dz;
    if (zs >= zlo && zs <= zhi) consider(b, ts, id, 0, near);
  }
  if (dz < 0.f) {
    const float tc = zhi / dz;
    const float x = dx * tc - cx, y = tc - cy;
    if (x * x + y * y <= r2) consider(b, tc, id, 0, near);
  }
}

__device__ __forceinline__ float seg_d2(const float* r, float gx, float gy) {
  const float ax = r[0], ay = r[1], ex = r[2], ey = r[3], inv = r[4];
  const float qx = gx - ax, qy = gy - ay;
  const float dot = qx * ex + qy * ey;
  float u = dot * inv;
  u = u < 0.f ? 0.f : (u > 1.f ? 1.f : u);      // the clamped projection
  const float cx = qx - u * ex, cy = qy - u * ey;
  return cx * cx + cy * cy;
}

__global__ void __launch_bounds__(256) camera_render_kernel(const CamArgs a) {
  // all of the workgroup's LDS is dynamic and sized by the launch to the world it draws, so that a light world keeps the CU's
  // occupancy: the object list (room for n_obj records), the ground records (n_gnd), then the palette's rows as r | g << 8 | b << 16 with
  // the five face shades behind them, and the four waves' counts.  No static LDS: the base stays 16-byte aligned.
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  float* const s_obj = s_mem;
  float* const s_gnd = s_obj + a.n_obj * kObjWords;
  int* const s_pal = reinterpret_cast<int*>(s_gnd + a.n_gnd * kGndWords);
  int* const s_cnt = s_pal + kPalWords;
  const int s = blockIdx.z;
  if (a.hold != nullptr && a.hold[s] != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const int x1 = min(x0 + kTileW, a.W) - 1, y1 = min(y0 + kTileH, a.H) - 1;
  const float* tab = a.prims + (size_t)s * a.scene_words;
  const float* obj = tab + kHdrWords;
  const float* gnd = obj + (size_t)a.n_obj * kObjWords;

  // ---- the objects whose rectangle meets this tile, in index order ----
  bool keep = false;
  if (tid < a.n_obj) {
    const int32_t* h = reinterpret_cast<const int32_t*>(obj + (size_t)tid * kObjWords);
    keep = h[0] != 0 && h[1] <= x1 && h[2] >= x0 && h[3] <= y1 && h[4] >= y0;
  }
  const unsigned long long mask = __ballot(keep);
  if (lane == 0) s_cnt[wave] = __popcll(mask);
  if (tid < ADX_CAMERA_PALETTE) s_pal[tid] = a.palette[tid][0] | a.palette[tid][1] << 8 | a.palette[tid][2] << 16;
  if (tid >= 64 && tid < 69) s_pal[ADX_CAMERA_PALETTE + tid - 64] = a.shade[tid - 64];
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += s_cnt[w];
  const int n_list = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
  if (keep) {
    const int slot = base + __popcll(mask & ((1ull << lane) - 1ull));
    const float4* src = reinterpret_cast<const float4*>(obj + (size_t)tid * kObjWords);
    float4* dst = reinterpret_cast<float4*>(s_obj + slot * kObjWords);
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
  }
  // ---- the ground records, for a tile that reaches below the horizon ----
  const bool tile_ground = ((float)y1 + 0.5f) - (float)a.H * 0.5f > 0.f;
  if (tile_ground) {
    const float4* src = reinterpret_cast<const float4*>(gnd);
    float4* dst = reinterpret_cast<float4*>(s_gnd);
    for (int i = tid; i < a.n_gnd * 2; i += 256) dst[i] = src[i];
  }
  __syncthreads();

  const int u = x0 + lane;
  const bool col_ok = u < a.W;
  const float dx = (((float)u + 0.5f) - (float)a.W * 0.5f) * a.k;
  const float A2 = dx * dx + 1.f;
  const float inf = __builtin_inff();
  for (int r = 0; r < kRows; ++r) {
    const int v = y0 + wave + 4 * r;
    if (v >= a.H) break;      // uniform over the wave
    const float dz = -((((float)v + 0.5f) - (float)a.H * 0.5f) * a.k);
    Best b;
    b.t = inf;
    b.id = kSky << 8;
    b.aux = 0;
    if (dz < 0.f) {
      const float tg = a.hgt / (-dz);
      if (tg > a.near) {
        b.t = tg;
        b.id = kGround << 8;
      }
    }
    const bool has_ground = b.id != 0;
    for (int i = 0; i < n_list; ++i) {
      const float* rec = s_obj + i * kObjWords;
      const int id = reinterpret_cast<const int32_t*>(rec)[0];
      const int cls = id >> 8;
      if (cls == kBox) {
        const float ax = rec[5], ay = rec[6];
        const float p = dx * ay;
        const float dl = dx * ax + ay, dw = ax - p;
        float tn = -inf, tf = inf;
        int face = 0;
        bool ok = true;
        slab(dl, rec[7], rec[8], 0, tn, tf, face, ok);
        slab(dw, rec[9], rec[10], 1, tn, tf, face, ok);
        slab(dz, rec[11], rec[12], 2, tn, tf, face, ok);
        if (ok && tn <= tf) consider(b, tn, face << 16 | id, 0, a.near);
      } else if (cls == kLamp) {
        const float lx = rec[5], ly = rec[6], lz = rec[7], R2 = rec[8];
        const float A3 = A2 + dz * dz;
        const float B = (dx * lx + ly) + dz * lz;
        const float c0 = ly * dz - lz, c1 = lz * dx - lx * dz, c2 = lx - ly * dx;      // the centre x the direction
        const float n2 = (c0 * c0 + c1 * c1) + c2 * c2;
        const float q = A3 * R2;
        const float disc = q - n2;
        if (disc >= 0.f) {
          const float sq = __builtin_sqrtf(disc);
          consider(b, (B - sq) / A3, id, reinterpret_cast<const int32_t*>(rec)[9], a.near);
        }
      } else {
        hit_cylinder(b, rec, id, dx, dz, A2, a.near);
      }
    }
    // ---- the ground's class, where the ground won ----
    if (has_ground && b.id == kGround << 8) {
      if (b.t > a.far) {
        b.id = kGround << 8 | 1;
      } else {
        const float gx = dx * b.t, gy = b.t;
        int cls = 0, slot = 0;
        for (int j = 0; j < a.NS; ++j) {
          const float* rec = s_gnd + j * kGndWords;
          if (reinterpret_cast<const int32_t*>(rec)[5] == 0) continue;
          const float d2 = seg_d2(rec, gx, gy);
          if (cls == 0 && d2 <= a.line2) {
            cls = kLine;
            slot = j;
          }
        }
        if (cls == 0) {
          float dmin = inf;
          for (int j = a.NS; j < a.n_gnd; ++j) {
            const float* rec = s_gnd + j * kGndWords;
            if (reinterpret_cast<const int32_t*>(rec)[5] == 0) continue;
            const float d2 = seg_d2(rec, gx, gy);
            if (d2 < dmin) dmin = d2;
          }
          cls = dmin < a.r_in2 ? kRoad : (dmin <= a.r_out2 ? kMark : kGround);
        }
        b.id = cls << 8 | slot;
      }
    }
    // ---- the colour: a pure function of the id and the phase ----
    const int cls = (b.id >> 8) & 0xff, slot = b.id & 0xff, face = b.id >> 16;
    int row;
    switch (cls) {
      case kSky: row = 0; break;
      case kGround: row = 1 + slot; break;
      case kRoad: row = 3; break;
      case kMark: row = 4; break;
      case kLine: row = 5; break;
      case kBox: row = 6 + (slot & 7); break;
      case kDisc: row = 14; break;
      case kPole: row = 15; break;
      default: row = 16 + ((b.aux - 1) & 3); break;
    }
    const int prgb = s_pal[row], sh = cls == kBox ? s_pal[ADX_CAMERA_PALETTE + face] : 256;
    int c[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[ch] = (((prgb >> (8 * ch)) & 0xff) * sh) >> 8;      // a box face: (c * shade[face]) >> 8
    const size_t pix = ((size_t)s * a.H + v) * a.W + u;
    if (a.frames != nullptr) {
      // a full row of 64 pixels is 48 words; they go out packed when the row's first byte is word-aligned
      uint8_t* rowp = a.frames + (((size_t)s * a.H + v) * a.W + x0) * 3;
      const bool pack = x0 + kTileW <= a.W && (reinterpret_cast<uintptr_t>(rowp) & 3u) == 0;
      const int rgb = c[0] | c[1] << 8 | c[2] << 16;
      if (pack) {
        const int p0 = (4 * lane) / 3, off = (4 * lane) - 3 * p0;
        const unsigned long long q0 = (unsigned)__shfl(rgb, p0 & 63, 64), q1 = (unsigned)__shfl(rgb, (p0 + 1) & 63, 64);
        if (lane < 48) reinterpret_cast<uint32_t*>(rowp)[lane] = (uint32_t)((q0 | q1 << 24) >> (8 * off));
      } else if (col_ok) {
        uint8_t* o = a.frames + pix * 3;
        o[0] = (uint8_t)c[0]; o[1] = (uint8_t)c[1]; o[2] = (uint8_t)c[2];
      }
    }
    if (col_ok) {
      if (a.image != nullptr) {
        const size_t hw = (size_t)a.H * a.W;
        float* o = a.image + (size_t)s * 3 * hw + (size_t)v * a.W + u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {      // adx_image_normalize's arithmetic
          const float f = (float)c[ch] / 255.0f;
          o[ch * hw] = (f - a.mean[ch]) / a.stdv[ch];
        }
      }
      if (a.ids != nullptr) a.ids[pix] = b.id;
      if (a.depth != nullptr) a.depth[pix] = b.t;
    }
  }
}

bool finite_pos(double v) { return v > 0.0 && v < __builtin_inf(); }
bool finite_nonneg(double v) { return v >= 0.0 && v < __builtin_inf(); }
bool finite_any(double v) { return v > -__builtin_inf() && v < __builtin_inf(); }

// the configuration's own ranges; what `who` names goes in front of every text
int camera_cfg_check(const adx_camera_cfg* c) {
  ADX_REQUIRE(c != nullptr, "camera: null configuration");
  ADX_REQUIRE(c->scenes >= 1 && c->scenes <= kCamMaxScenes, "camera: %d scenes, supported 1..%d", c->scenes, kCamMaxScenes);
  ADX_REQUIRE(c->width >= 8 && c->width <= 2048, "camera: width %d, supported 8..2048", c->width);
  ADX_REQUIRE(c->height >= 8 && c->height <= 1024, "camera: height %d, supported 8..1024", c->height);
  ADX_REQUIRE(c->n_boxes >= 0 && c->n_boxes <= kCamMaxSlots, "camera: %d boxes, supported 0..%d", c->n_boxes, kCamMaxSlots);
  ADX_REQUIRE(c->n_discs >= 0 && c->n_discs <= kCamMaxSlots, "camera: %d discs, supported 0..%d", c->n_discs, kCamMaxSlots);
  ADX_REQUIRE(c->n_signals >= 0 && c->n_signals <= kCamMaxSlots, "camera: %d signals, supported 0..%d", c->n_signals, kCamMaxSlots);
  ADX_REQUIRE(c->n_paths >= 0 && c->n_paths <= kCamMaxPaths, "camera: %d paths, supported 0..%d", c->n_paths, kCamMaxPaths);
  ADX_REQUIRE(c->n_paths == 0 ? c->n_points == 0 : (c->n_points >= 2 && c->n_points <= kCamMaxPoints),
              "camera: %d points per path, supported 2..%d (0 without paths)", c->n_points, kCamMaxPoints);
  ADX_REQUIRE(c->fov > 0.0 && c->fov < 3.0, "camera: fov %g must lie in (0, 3) rad", c->fov);
  ADX_REQUIRE(finite_any(c->mount_back), "camera: mount_back %g must be finite", c->mount_back);
  ADX_REQUIRE(finite_pos(c->cam_height), "camera: cam_height %g must be finite and > 0", c->cam_height);
  ADX_REQUIRE(finite_pos(c->near), "camera: near %g must be finite and > 0", c->near);
  ADX_REQUIRE(finite_pos(c->far) && c->far > c->near, "camera: far %g must be finite and > near", c->far);
  ADX_REQUIRE(finite_pos(c->half_width), "camera: half_width %g must be finite and > 0", c->half_width);
  ADX_REQUIRE(finite_nonneg(c->mark) && c->mark <= c->half_width, "camera: mark %g must lie in 0..half_width", c->mark);
  ADX_REQUIRE(finite_pos(c->line_half), "camera: line_half %g must be finite and > 0", c->line_half);
  ADX_REQUIRE(finite_pos(c->box_height), "camera: box_height %g must be finite and > 0", c->box_height);
  ADX_REQUIRE(finite_pos(c->disc_height), "camera: disc_height %g must be finite and > 0", c->disc_height);
  ADX_REQUIRE(finite_pos(c->lamp_radius), "camera: lamp_radius %g must be finite and > 0", c->lamp_radius);
  ADX_REQUIRE(finite_pos(c->lamp_height), "camera: lamp_height %g must be finite and > 0", c->lamp_height);
  ADX_REQUIRE(finite_any(c->lamp_setback), "camera: lamp_setback %g must be finite", c->lamp_setback);
  ADX_REQUIRE(finite_nonneg(c->pole_radius), "camera: pole_radius %g must be finite and >= 0", c->pole_radius);
  for (int i = 0; i < 3; ++i) {
    ADX_REQUIRE(finite_any((double)c->mean[i]), "camera: mean[%d] %g must be finite", i, (double)c->mean[i]);
    ADX_REQUIRE(finite_any((double)c->stdv[i]) && c->stdv[i] != 0.f, "camera: std[%d] %g must be finite and not 0", i, (double)c->stdv[i]);
  }
  return ADX_OK;
}

size_t scene_words(const adx_camera_cfg* c) {
  const int n_obj = c->n_boxes + c->n_discs + 2 * c->n_signals;
  const int n_gnd = c->n_signals + c->n_paths * (c->n_paths == 0 ? 0 : c->n_points - 1);
  return (size_t)kHdrWords + (size_t)kObjWords * n_obj + (size_t)kGndWords * n_gnd;
}

}  // namespace

size_t camera_prims_bytes(const adx_camera_cfg* c) {
  if (c == nullptr || c->scenes < 1 || c->scenes > kCamMaxScenes || c->n_boxes < 0 || c->n_boxes > kCamMaxSlots || c->n_discs < 0 ||
      c->n_discs > kCamMaxSlots || c->n_signals < 0 || c->n_signals > kCamMaxSlots || c->n_paths < 0 || c->n_paths > kCamMaxPaths ||
      (c->n_paths == 0 ? c->n_points != 0 : (c->n_points < 2 || c->n_points > kCamMaxPoints)))
    return 0;
  return (size_t)c->scenes * scene_words(c) * sizeof(float);
}

void camera_default_palette(uint8_t* palette, uint8_t* shade) {
  static const uint8_t rows[ADX_CAMERA_PALETTE][3] = {
      {135, 190, 235},                                                                                    // sky
      {96, 128, 72},   {120, 140, 110},                                                                   // ground, far ground
      {70, 70, 74},    {230, 230, 225}, {250, 250, 250},                                                  // road, marking, stop line
      {200, 40, 40},   {40, 80, 200},   {230, 200, 40}, {240, 240, 240}, {30, 30, 30},  {40, 160, 80},    // boxes j % 8
      {150, 90, 170},  {230, 130, 40},
      {150, 110, 70},                                                                                     // disc
      {60, 60, 60},                                                                                       // pole
      {30, 220, 60},   {250, 210, 30},  {240, 30, 30},  {250, 120, 20}};                                  // lamp: green, yellow, red, sign
  static const uint8_t faces[5] = {200, 232, 168, 184, 255};      // -length, +length, -width, +width, top
  if (palette != nullptr)
    for (int i = 0; i < ADX_CAMERA_PALETTE; ++i)
      for (int ch = 0; ch < 3; ++ch) palette[i * 3 + ch] = rows[i][ch];
  if (shade != nullptr)
    for (int i = 0; i < 5; ++i) shade[i] = faces[i];
}

int camera_render(const adx_camera_cfg* c, const double* pose, const double* boxes, const double* discs, const double* signals,
                  const int32_t* phase, const double* roads, const int32_t* road_len, const int32_t* hold, void* prims, uint8_t* frames,
                  float* image, int32_t* ids, float* depth, hipStream_t s) {
  const int rc = camera_cfg_check(c);
  if (rc != ADX_OK) return rc;
  const int S = c->scenes, W = c->width, H = c->height, NB = c->n_boxes, ND = c->n_discs, NS = c->n_signals, Q = c->n_paths, G = c->n_points;
  ADX_REQUIRE(pose != nullptr, "camera: null pose");
  ADX_REQUIRE(NB == 0 || boxes != nullptr, "camera: null boxes with n_boxes = %d", NB);
  ADX_REQUIRE(ND == 0 || discs != nullptr, "camera: null discs with n_discs = %d", ND);
  ADX_REQUIRE(NS == 0 || signals != nullptr, "camera: null signals with n_signals = %d", NS);
  ADX_REQUIRE(NS == 0 || phase != nullptr, "camera: null phase with n_signals = %d", NS);
  ADX_REQUIRE(Q == 0 || roads != nullptr, "camera: null roads with n_paths = %d", Q);
  ADX_REQUIRE(Q == 0 || road_len != nullptr, "camera: null road_len with n_paths = %d", Q);
  ADX_REQUIRE(prims != nullptr, "camera: null prims");
  ADX_REQUIRE((reinterpret_cast<uintptr_t>(prims) & 15u) == 0, "camera: prims must be 16-byte aligned");
  ADX_REQUIRE(frames != nullptr || image != nullptr || ids != nullptr || depth != nullptr, "camera: no output (frames, image, ids, depth all null)");
  const size_t px = (size_t)S * H * W;
  const ByteSpan ins[8] = {{pose, (size_t)S * 3 * sizeof(double)},
                           {NB ? boxes : nullptr, (size_t)S * NB * 7 * sizeof(double)},
                           {ND ? discs : nullptr, (size_t)S * ND * 5 * sizeof(double)},
                           {NS ? signals : nullptr, (size_t)S * NS * 10 * sizeof(double)},
                           {NS ? phase : nullptr, (size_t)S * NS * sizeof(int32_t)},
                           {Q ? roads : nullptr, (size_t)S * Q * G * 2 * sizeof(double)},
                           {Q ? road_len : nullptr, (size_t)S * Q * sizeof(int32_t)},
                           {hold, (size_t)S * sizeof(int32_t)}};
  const char* const in_names[8] = {"pose", "boxes", "discs", "signals", "phase", "roads", "road_len", "hold"};
  const ByteSpan outs[5] = {{prims, camera_prims_bytes(c)}, {frames, px * 3}, {image, px * 3 * sizeof(float)}, {ids, px * sizeof(int32_t)},
                            {depth, px * sizeof(float)}};
  const char* const names[5] = {"prims", "frames", "image", "ids", "depth"};
  for (int i = 0; i < 5; ++i) {
    if (outs[i].p == nullptr) continue;
    for (int j = 0; j < 8; ++j)
      ADX_REQUIRE(ins[j].p == nullptr || !byte_ranges_overlap(outs[i].p, outs[i].n, ins[j].p, ins[j].n), "camera: %s aliases %s", names[i],
                  in_names[j]);
    for (int j = 0; j < i; ++j)
      ADX_REQUIRE(outs[j].p == nullptr || !byte_ranges_overlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n),
                  "camera: %s and %s alias each other", names[j], names[i]);
  }
  CamArgs a = {};
  a.pose = pose; a.boxes = boxes; a.discs = discs; a.signals = signals; a.roads = roads;
  a.phase = phase; a.road_len = road_len; a.hold = hold;
  a.prims = static_cast<float*>(prims);
  a.frames = frames; a.image = image; a.ids = ids; a.depth = depth;
  a.W = W; a.H = H; a.NB = NB; a.ND = ND; a.NS = NS; a.Q = Q; a.G = G;
  a.n_obj = NB + ND + 2 * NS;
  a.n_gnd = NS + Q * (Q == 0 ? 0 : G - 1);
  a.scene_words = (int)scene_words(c);
  a.k = (float)(2.0 * tan(c->fov / 2.0) / (double)W);      // formed in fp64, rounded once
  a.k64 = (double)a.k;
  a.mount_back = c->mount_back; a.height = c->cam_height; a.box_height = c->box_height; a.disc_height = c->disc_height;
  a.lamp_radius = c->lamp_radius; a.lamp_height = c->lamp_height; a.lamp_setback = c->lamp_setback; a.pole_radius = c->pole_radius;
  a.hgt = (float)c->cam_height; a.near = (float)c->near; a.far = (float)c->far;
  a.r_in2 = (float)((c->half_width - c->mark) * (c->half_width - c->mark));
  a.r_out2 = (float)(c->half_width * c->half_width);
  a.line2 = (float)(c->line_half * c->line_half);
  for (int i = 0; i < 3; ++i) {
    a.mean[i] = c->mean[i];
    a.stdv[i] = c->stdv[i];
  }
  for (int i = 0; i < ADX_CAMERA_PALETTE; ++i)
    for (int ch = 0; ch < 3; ++ch) a.palette[i][ch] = c->palette[i][ch];
  for (int i = 0; i < 5; ++i) a.shade[i] = c->shade[i];
  camera_stage_kernel<<<dim3(S), dim3(64), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  const size_t lds = (size_t)(a.n_obj * kObjWords + a.n_gnd * kGndWords + kPalWords + 4) * sizeof(float);
  static_assert(ADX_CAMERA_PALETTE + 5 <= kPalWords, "camera v1: the palette's LDS words");
  camera_render_kernel<<<dim3(ceil_div(W, kTileW), ceil_div(H, kTileH), S), dim3(256), lds, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

}  // namespace adx
