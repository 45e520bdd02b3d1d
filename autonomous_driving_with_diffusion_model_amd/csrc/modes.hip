// Trajectory modes (include/adx.h: adx_traj_modes, "trajectory modes v1"): a greedy cover of a scene's K candidates under a radius.
// No reference counterpart: the reference's train.evaluate draws many trajectories for one image only to paint them
// (train.py:62-90).
//
// One workgroup per scene, 256 threads = 4 waves.  The scene's scored xy are staged in LDS as two planes (x, y) with a candidate
// stride of 65 words: in the distance pass lane j reads candidate j's waypoint h at word j * 65 + h, and an odd stride puts the
// 32 lanes of each half of the wave (a 4-byte read is served half by half, 32 banks wide) on 32 different banks.  Then
//   1. every wave forms the 64-bit mask of the finite candidates (lane = candidate, a ballot);
//   2. the distances: wave w owns the rows i = w, w + 4, ...; lane = j.  It walks h = h0 .. H-1 in that order, p_i a broadcast
//      read and p_j the lane's own, divides by n and one ballot of `near` gives row i's adjacency as one 64-bit mask, kept in LDS;
//   3. the cover, in the first wave alone (lane = candidate) over those K masks and a 64-bit alive mask every lane holds: n_i is a
//      popcount of adj[i] & alive, the arg-max a butterfly that breaks ties to the lower lane; M rounds, no block-wide barrier;
//   4. all threads copy the M representative rows word for word.
// No atomics and no inter-workgroup traffic: a given input gives the same bits on every launch.  Every product and sum is rounded
// on its own (no contraction), so dist2[i][j] and dist2[j][i] hold the same bits: (-d) * (-d) is d * d.
#include "sched.h"

namespace adx {

namespace {

constexpr int kModMaxK = 64, kModMaxM = 64, kModMaxH = 64, kModMaxD = 16, kModWaves = 4;
constexpr int kModStride = kModMaxH + 1;      // odd: lanes holding different candidates hit different banks

struct ModesArgs {
  const float* trajs;
  float* modes;
  int32_t* index;     // [scenes][M]
  int32_t* mass;      // [scenes][M]
  int32_t* assign;    // [scenes][K]
  int32_t* count;     // [scenes]
  float* dist2;       // [scenes][K][K] or null
  int scenes, K, H, D, M, h0;
  float r2;
};

__global__ void __launch_bounds__(256) traj_modes_kernel(const ModesArgs a) {
#pragma clang fp contract(off)
  __shared__ float xs[kModMaxK * kModStride], ys[kModMaxK * kModStride];
  __shared__ unsigned long long adj_s[kModMaxK];
  __shared__ int rep_s[kModMaxM];
  __shared__ int count_s;
  const int s = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int K = a.K, H = a.H, D = a.D, M = a.M, h0 = a.h0;
  const int n = H - h0;
  const size_t row_floats = (size_t)H * D;

  // stage the scored waypoints: element i = k * n + (h - h0) of the scene; candidate k of scene s is row k * scenes + s
  for (int i = tid; i < K * n; i += 256) {
    const int k = i / n, hh = i - k * n;
    const float* p = a.trajs + ((size_t)k * a.scenes + s) * row_floats + (size_t)(h0 + hh) * D;
    xs[k * kModStride + hh] = p[0];
    ys[k * kModStride + hh] = D > 1 ? p[1] : 0.f;
  }
  __syncthreads();

  // 1. the finite candidates (every wave forms the same mask: no barrier for it)
  const bool in = lane < K;
  const int own = lane * kModStride;      // lanes >= K never read
  bool fin = in;
  if (in)
    for (int hh = 0; hh < n; ++hh) fin = fin && finite_f(xs[own + hh]) && finite_f(ys[own + hh]);
  const unsigned long long finite = __ballot(fin);

  // 2. distances and adjacency.  Wave-uniform trip count: the ballot sees all 64 lanes
  const float nf = (float)n;
  for (int i = wave; i < K; i += kModWaves) {
    const int base = i * kModStride;
    float d = 0.f;
    if (in) {
      float acc = 0.f;
      for (int hh = 0; hh < n; ++hh) {
        const float dx = xs[base + hh] - xs[own + hh], dy = ys[base + hh] - ys[own + hh];
        acc = acc + (dx * dx + dy * dy);
      }
      d = acc / nf;
      if (a.dist2 != nullptr) a.dist2[((size_t)s * K + i) * K + lane] = d;
    }
    const bool near = fin && ((finite >> i) & 1ull) != 0ull && d <= a.r2;
    const unsigned long long row = __ballot(near);
    if (lane == 0) adj_s[i] = row;
  }
  __syncthreads();

  // 3. the greedy cover: lane = candidate, `alive` is the same word in every lane
  if (wave == 0) {
    const unsigned long long mine = in ? adj_s[lane] : 0ull;
    unsigned long long alive = finite;
    int label = in ? (fin ? -1 : -2) : 0;
    int count = 0;
    for (int m = 0; m < M; ++m) {
      int c = ((alive >> lane) & 1ull) != 0ull ? __popcll(mine & alive) : 0;
      int idx = lane;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const int oc = __shfl_xor(c, off, 64);
        const int oi = __shfl_xor(idx, off, 64);
        if (oc > c || (oc == c && oi < idx)) { c = oc; idx = oi; }
      }
      if (c == 0) break;      // nothing alive (an alive candidate counts itself); uniform: every lane holds the same c
      const unsigned long long cover = adj_s[idx] & alive;      // idx < K: its count is positive
      if (((cover >> lane) & 1ull) != 0ull) label = m;
      alive &= ~cover;
      if (lane == 0) {
        rep_s[m] = idx;
        a.index[(size_t)s * M + m] = idx;
        a.mass[(size_t)s * M + m] = c;
      }
      count = m + 1;
    }
    if (lane >= count && lane < M) {      // M <= 64: one lane per empty slot
      a.index[(size_t)s * M + lane] = -1;
      a.mass[(size_t)s * M + lane] = 0;
    }
    if (in) a.assign[(size_t)s * K + lane] = label;
    if (lane == 0) {
      count_s = count;
      a.count[s] = count;
    }
  }
  __syncthreads();

  // 4. the representatives' full [H][D] rows, bit for bit; a slot without a mode repeats mode 0, no mode at all: zeros
  const int count = count_s;
  const int words = H * D;
  for (int m = 0; m < M; ++m) {
    uint32_t* dst = reinterpret_cast<uint32_t*>(a.modes + ((size_t)m * a.scenes + s) * row_floats);
    if (count == 0) {
      for (int i = tid; i < words; i += 256) dst[i] = 0u;
      continue;
    }
    const int rep = rep_s[m < count ? m : 0];
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.trajs + ((size_t)rep * a.scenes + s) * row_floats);
    for (int i = tid; i < words; i += 256) dst[i] = src[i];
  }
}

}  // namespace

int traj_modes(const adx_modes_cfg* c, const float* trajs, float* modes, int32_t* index, int32_t* mass, int32_t* assign,
               int32_t* count, float* dist2, hipStream_t s) {
  ADX_REQUIRE(c != nullptr, "traj modes: null configuration");
  const int S = c->scenes, K = c->candidates, H = c->horizon, D = c->dim, M = c->max_modes;
  ADX_REQUIRE(K >= 1 && K <= kModMaxK, "traj modes: %d candidates, supported 1..%d", K, kModMaxK);
  ADX_REQUIRE(M >= 1 && M <= kModMaxM, "traj modes: max_modes %d, supported 1..%d", M, kModMaxM);
  ADX_REQUIRE(H >= 1 && H <= kModMaxH, "traj modes: horizon %d, supported 1..%d", H, kModMaxH);
  ADX_REQUIRE(D >= 1 && D <= kModMaxD, "traj modes: transition dim %d, supported 1..%d", D, kModMaxD);
  ADX_REQUIRE(S >= 1 && S <= 65535, "traj modes: %d scenes, supported 1..65535", S);
  ADX_REQUIRE(c->h0 >= 0 && c->h0 <= H - 1, "traj modes: h0 %d, supported 0..%d (horizon - 1)", c->h0, H - 1);
  ADX_REQUIRE(finite_f(c->radius) && c->radius >= 0.f, "traj modes: radius %g must be finite and >= 0", (double)c->radius);
  ADX_REQUIRE(trajs != nullptr, "traj modes: null trajs");
  ADX_REQUIRE(modes != nullptr, "traj modes: null modes");
  ADX_REQUIRE(index != nullptr, "traj modes: null index");
  ADX_REQUIRE(mass != nullptr, "traj modes: null mass");
  ADX_REQUIRE(assign != nullptr, "traj modes: null assign");
  ADX_REQUIRE(count != nullptr, "traj modes: null count");
  const size_t row = (size_t)H * D * sizeof(float);
  const size_t in_bytes = (size_t)K * S * row;
  const ByteSpan outs[6] = {{modes, (size_t)M * S * row},
                            {index, (size_t)S * M * sizeof(int32_t)},
                            {mass, (size_t)S * M * sizeof(int32_t)},
                            {assign, (size_t)S * K * sizeof(int32_t)},
                            {count, (size_t)S * sizeof(int32_t)},
                            {dist2, (size_t)S * K * K * sizeof(float)}};
  const char* const names[6] = {"modes", "index", "mass", "assign", "count", "dist2"};
  for (int i = 0; i < 6; ++i) {
    if (outs[i].p == nullptr) continue;      // dist2 alone may be
    ADX_REQUIRE(!byte_ranges_overlap(outs[i].p, outs[i].n, trajs, in_bytes), "traj modes: %s aliases trajs", names[i]);
    for (int j = 0; j < i; ++j)
      ADX_REQUIRE(!byte_ranges_overlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n), "traj modes: %s and %s alias each other",
                  names[j], names[i]);
  }
  ModesArgs a = {};
  a.trajs = trajs; a.modes = modes; a.index = index; a.mass = mass; a.assign = assign; a.count = count; a.dist2 = dist2;
  a.scenes = S; a.K = K; a.H = H; a.D = D; a.M = M; a.h0 = c->h0;
  a.r2 = c->radius * c->radius;      // rounded once
  traj_modes_kernel<<<dim3(S), dim3(256), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

}  // namespace adx
