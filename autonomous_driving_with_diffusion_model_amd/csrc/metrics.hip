// Open-loop metrics (include/adx.h: adx_traj_metrics, adx_metrics_accumulate, "open-loop metrics v1"): ADE / FDE of the chosen
// plan, minADE_K / minFDE_K over a scene's candidates, miss flags, the along / cross split of the final error and the displacement
// per waypoint, against logged waypoints.  No reference counterpart: the reference's train.evaluate paints dots (train.py:62-90).
//
// traj_metrics_kernel has the shape of select.hip: one workgroup per scene, 256 threads = 4 waves.  The scene's K x H xy pairs are
// staged in LDS as two planes (every later read is a 4-byte read at consecutive lanes = consecutive banks), the logged waypoints
// beside them.  Then
//   1. wave w walks candidates k = w, w + 4, ... with lane = waypoint: the displacement, its sum over the wave by the fixed xor
//      butterfly (every lane ends with the same value; the tree does not depend on K, on the scored range or on the launch), the
//      final displacement by one shuffle; the wave that meets the chosen candidate also writes its row of disp_sel and leaves the
//      final error vector in LDS;
//   2. the first wave's two searches over the K results (lane = candidate), ties and non-finite values by the rule of selection
//      cost v1 (restated here: select.hip keeps its code), and lane 0 writes the record.
// No atomics and no inter-workgroup traffic: a given input gives the same bits on every launch.  Every product, sum, division and
// square root is rounded on its own (no contraction).  Latency-sized like select.hip: no occupancy or bandwidth target applies.
//
// metrics_accumulate_kernel is one workgroup; thread t owns word t of the state and walks the scenes in index order in fp64, so the
// state's bits depend on the batches and their order alone.  Counts and sums leave through ordinary vector stores.
#include "sched.h"

#pragma clang fp contract(off)      // the whole file: the helpers below are part of the contract's arithmetic too

namespace adx {

namespace {

constexpr int kMetMaxK = 64, kMetMaxH = 64, kMetWaves = 4;
// the state: 16 head words, then per waypoint a sum and a count (adx.h lists them)
constexpr int kAccHead = 16, kAccWords = kAccHead + 2 * kMetMaxH;
constexpr int kAccScored = 0, kAccNonFinite = 1, kAccHeading = 2, kAccAgree = 3, kAccBlocked = 4, kAccRec = 5, kAccRegret = 13,
              kAccAlong = 14, kAccCross = 15, kAccDisp = kAccHead, kAccDispCount = kAccHead + kMetMaxH;

struct MetricsArgs {
  const float* trajs;
  const float* gt;
  const int32_t* valid;    // [scenes] or null
  const int32_t* index;    // [scenes] or null
  float* ade;
  float* fde;
  int32_t* best;
  float* rec;
  int32_t* flags;
  float* disp_sel;
  int scenes, K, H, D, h0;
  float miss_radius, xy_scale;
};

// the smallest k among the smallest finite values (lane = candidate); no finite value at all -> every key is +inf -> k = 0
__device__ __forceinline__ int wave_argmin_finite(float c, bool in, int lane) {
  float v = __builtin_inff();
  int idx = lane;
  if (in && finite_f(c)) v = c;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off, kWave);
    const int oi = __shfl_xor(idx, off, kWave);
    if (ov < v || (ov == v && oi < idx)) { v = ov; idx = oi; }
  }
  return idx;
}

__global__ void __launch_bounds__(kMetWaves* kWave) traj_metrics_kernel(const MetricsArgs a) {
  __shared__ float xs[kMetMaxK * kMetMaxH], ys[kMetMaxK * kMetMaxH];
  __shared__ float gx_s[kMetMaxH], gy_s[kMetMaxH];
  __shared__ float ade_s[kMetMaxK], fde_s[kMetMaxK];
  __shared__ float sel_e[2];
  const int s = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & (kWave - 1);
  const int K = a.K, H = a.H, D = a.D, h0 = a.h0;
  int n = a.valid != nullptr ? a.valid[s] : H;
  n = n < 0 ? 0 : (n > H ? H : n);
  const int sel = a.index != nullptr ? a.index[s] : 0;

  if (!(n > h0 && sel >= 0 && sel < K)) {      // the whole workgroup alike: an unscored scene is zeros, and no barrier is met
    for (int k = tid; k < K; k += kMetWaves * kWave) { a.ade[(size_t)s * K + k] = 0.f; a.fde[(size_t)s * K + k] = 0.f; }
    if (tid < H) a.disp_sel[(size_t)s * H + tid] = 0.f;
    if (tid < ADX_METRICS_REC) a.rec[(size_t)s * ADX_METRICS_REC + tid] = 0.f;
    if (tid == 0) { a.best[s] = 0; a.flags[s] = 0; }
    return;
  }

  // stage: element i = k * H + h of the scene; candidate k of scene s is row k * scenes + s
  const size_t row_floats = (size_t)H * D;
  for (int i = tid; i < K * H; i += kMetWaves * kWave) {
    const int k = i / H, h = i - k * H;
    const float* p = a.trajs + ((size_t)k * a.scenes + s) * row_floats + (size_t)h * D;
    xs[i] = p[0];
    ys[i] = p[1];
  }
  if (tid < H) {
    gx_s[tid] = a.gt[((size_t)s * H + tid) * 2];
    gy_s[tid] = a.gt[((size_t)s * H + tid) * 2 + 1];
  }
  __syncthreads();

  // 1. per candidate: lane = waypoint, the lanes outside the scored range hold 0
  const bool live = lane >= h0 && lane < n;
  const float gx = live ? gx_s[lane] : 0.f, gy = live ? gy_s[lane] : 0.f;
  const float count = (float)(n - h0);
  for (int k = wave; k < K; k += kMetWaves) {      // wave-uniform trip count: the shuffles below see all 64 lanes
    float ex = 0.f, ey = 0.f, disp = 0.f;
    if (live) {
      ex = (xs[k * H + lane] - gx) * a.xy_scale;
      ey = (ys[k * H + lane] - gy) * a.xy_scale;
      disp = sqrtf(ex * ex + ey * ey);
    }
    const float ade = wave_sum(disp) / count;
    const float fde = __shfl(disp, n - 1, kWave);
    if (lane == 0) {
      ade_s[k] = ade;
      fde_s[k] = fde;
      a.ade[(size_t)s * K + k] = ade;
      a.fde[(size_t)s * K + k] = fde;
    }
    if (k == sel) {
      if (lane < H) a.disp_sel[(size_t)s * H + lane] = disp;
      if (lane == n - 1) { sel_e[0] = ex; sel_e[1] = ey; }
    }
  }
  __syncthreads();

  // 2. the searches and the record
  if (wave == 0) {
    const bool in = lane < K;
    const int best = wave_argmin_finite(in ? ade_s[lane] : 0.f, in, lane);
    const int best_f = wave_argmin_finite(in ? fde_s[lane] : 0.f, in, lane);
    if (lane == 0) {
      const float min_ade = ade_s[best], min_fde = fde_s[best_f], sel_ade = ade_s[sel], sel_fde = fde_s[sel];
      float along = 0.f, cross = 0.f;
      int flags = ADX_METRICS_FLAG_SCORED | (n << 8) | (h0 << 16);
      if (n - h0 >= 2) {
        const float dx = gx_s[n - 1] - gx_s[n - 2], dy = gy_s[n - 1] - gy_s[n - 2];
        const float len = sqrtf(dx * dx + dy * dy);
        if (len > 0.f && len < __builtin_inff()) {
          const float ux = dx / len, uy = dy / len;
          along = sel_e[0] * ux + sel_e[1] * uy;
          cross = sel_e[1] * ux - sel_e[0] * uy;
          flags |= ADX_METRICS_FLAG_HEADING;
        }
      }
      if (finite_f(sel_ade)) flags |= ADX_METRICS_FLAG_FINITE;
      float* r = a.rec + (size_t)s * ADX_METRICS_REC;
      r[0] = min_ade; r[1] = min_fde; r[2] = sel_ade; r[3] = sel_fde; r[4] = along; r[5] = cross;
      r[6] = sel_fde > a.miss_radius ? 1.f : 0.f;
      r[7] = min_fde > a.miss_radius ? 1.f : 0.f;
      a.best[s] = best;
      a.flags[s] = flags;
    }
  }
}

struct AccumulateArgs {
  void* state;
  const float* rec;
  const int32_t* flags;
  const int32_t* best;
  const int32_t* index;      // or null: candidate 0
  const float* disp_sel;
  const int32_t* blocked;    // or null
  int scenes, H;
};

__global__ void __launch_bounds__(256) metrics_accumulate_kernel(const AccumulateArgs a) {
  const int t = threadIdx.x;
  if (t >= kAccWords) return;
  const int h = t >= kAccDispCount ? t - kAccDispCount : t - kAccDisp;      // of the per-waypoint words
  if (t >= kAccHead && h >= a.H) return;
  const bool counts = t <= kAccBlocked || t >= kAccDispCount;               // an int64 word; the others are fp64
  double* fw = static_cast<double*>(a.state) + t;
  int64_t* iw = static_cast<int64_t*>(a.state) + t;
  double fs = counts ? 0.0 : *fw;
  int64_t is = counts ? *iw : 0;
  for (int s = 0; s < a.scenes; ++s) {
    const int f = a.flags[s];
    if ((f & ADX_METRICS_FLAG_SCORED) == 0) continue;
    const bool finite = (f & ADX_METRICS_FLAG_FINITE) != 0;
    if (t == kAccScored) { ++is; continue; }
    if (t == kAccNonFinite) { is += finite ? 0 : 1; continue; }
    if (!finite) continue;                  // counted above, summed nowhere
    const float* r = a.rec + (size_t)s * ADX_METRICS_REC;
    const bool heading = (f & ADX_METRICS_FLAG_HEADING) != 0;
    if (t == kAccHeading) is += heading ? 1 : 0;
    else if (t == kAccAgree) is += a.best[s] == (a.index != nullptr ? a.index[s] : 0) ? 1 : 0;
    else if (t == kAccBlocked) is += (a.blocked != nullptr && a.blocked[s] != 0) ? 1 : 0;
    else if (t < kAccRegret) fs += (double)r[t - kAccRec];
    else if (t == kAccRegret) fs += (double)r[2] - (double)r[0];
    else if (t <= kAccCross) { if (heading) fs += __builtin_fabs((double)r[4 + (t - kAccAlong)]); }
    else {
      const int n = (f >> 8) & 0x7f, h0 = (f >> 16) & 0x7f;
      if (h >= h0 && h < n) {
        if (counts) ++is;
        else fs += (double)a.disp_sel[(size_t)s * a.H + h];
      }
    }
  }
  if (counts) *iw = is;
  else *fw = fs;
}

__global__ void __launch_bounds__(256) metrics_reset_kernel(uint64_t* state) {
  if ((int)threadIdx.x < kAccWords) state[threadIdx.x] = 0ull;
}

}  // namespace

size_t metrics_state_bytes() { return (size_t)kAccWords * sizeof(uint64_t); }

int traj_metrics(const adx_metrics_cfg* c, const float* trajs, const float* gt, const int32_t* valid, const int32_t* index, float* ade,
                 float* fde, int32_t* best, float* rec, int32_t* flags, float* disp_sel, hipStream_t s) {
  ADX_REQUIRE(c != nullptr, "traj metrics: null configuration");
  const int S = c->scenes, K = c->candidates, H = c->horizon, D = c->dim;
  ADX_REQUIRE(K >= 1 && K <= kMetMaxK, "traj metrics: %d candidates, supported 1..%d", K, kMetMaxK);
  ADX_REQUIRE(H >= 1 && H <= kMetMaxH, "traj metrics: horizon %d, supported 1..%d", H, kMetMaxH);
  ADX_REQUIRE(D >= 2, "traj metrics: the metrics score (x, y), dim is %d", D);
  ADX_REQUIRE(S >= 1 && S <= 65535, "traj metrics: %d scenes, supported 1..65535", S);
  const int rc = shape_check("traj metrics", K * S, H, D);
  if (rc != ADX_OK) return rc;
  ADX_REQUIRE(c->h0 >= 0 && c->h0 < H, "traj metrics: first scored waypoint %d, supported 0..%d (horizon %d)", c->h0, H - 1, H);
  ADX_REQUIRE(finite_f(c->xy_scale) && c->xy_scale > 0.f, "traj metrics: xy_scale must be finite and > 0, got %g", (double)c->xy_scale);
  ADX_REQUIRE(c->miss_radius >= 0.f, "traj metrics: miss_radius must be >= 0, got %g", (double)c->miss_radius);
  ADX_REQUIRE(trajs != nullptr && gt != nullptr, "traj metrics: null input");
  ADX_REQUIRE(ade != nullptr && fde != nullptr && best != nullptr && rec != nullptr && flags != nullptr && disp_sel != nullptr,
              "traj metrics: null output");
  const size_t sk = (size_t)S * K * sizeof(float), s4 = (size_t)S * sizeof(int32_t);
  const ByteSpan ins[4] = {{trajs, (size_t)K * S * H * D * sizeof(float)}, {gt, (size_t)S * H * 2 * sizeof(float)}, {valid, s4}, {index, s4}};
  const ByteSpan outs[6] = {{ade, sk}, {fde, sk}, {best, s4}, {rec, (size_t)S * ADX_METRICS_REC * sizeof(float)}, {flags, s4},
                            {disp_sel, (size_t)S * H * sizeof(float)}};
  for (int i = 0; i < 6; ++i) {
    for (int j = 0; j < 4; ++j)
      ADX_REQUIRE(ins[j].p == nullptr || !byte_ranges_overlap(outs[i].p, outs[i].n, ins[j].p, ins[j].n),
                  "traj metrics: an output overlaps an input");
    for (int j = 0; j < i; ++j)
      ADX_REQUIRE(!byte_ranges_overlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n), "traj metrics: outputs overlap each other");
  }
  MetricsArgs a;
  a.trajs = trajs; a.gt = gt; a.valid = valid; a.index = index;
  a.ade = ade; a.fde = fde; a.best = best; a.rec = rec; a.flags = flags; a.disp_sel = disp_sel;
  a.scenes = S; a.K = K; a.H = H; a.D = D; a.h0 = c->h0;
  a.miss_radius = c->miss_radius; a.xy_scale = c->xy_scale;
  traj_metrics_kernel<<<dim3(S), dim3(kMetWaves * kWave), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

int metrics_reset(void* state, hipStream_t s) {
  ADX_REQUIRE(state != nullptr, "metrics reset: null state");
  metrics_reset_kernel<<<dim3(1), dim3(256), 0, s>>>(static_cast<uint64_t*>(state));
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

int metrics_accumulate(void* state, const float* rec, const int32_t* flags, const int32_t* best, const int32_t* index,
                       const float* disp_sel, const int32_t* blocked, int scenes, int horizon, hipStream_t s) {
  ADX_REQUIRE(scenes >= 1 && scenes <= 65535, "metrics accumulate: %d scenes, supported 1..65535", scenes);
  ADX_REQUIRE(horizon >= 1 && horizon <= kMetMaxH, "metrics accumulate: horizon %d, supported 1..%d", horizon, kMetMaxH);
  ADX_REQUIRE(state != nullptr, "metrics accumulate: null state");
  ADX_REQUIRE(rec != nullptr && flags != nullptr && best != nullptr && disp_sel != nullptr, "metrics accumulate: null input");
  const size_t s4 = (size_t)scenes * sizeof(int32_t);
  const ByteSpan ins[6] = {{rec, (size_t)scenes * ADX_METRICS_REC * sizeof(float)}, {flags, s4}, {best, s4}, {index, s4},
                           {disp_sel, (size_t)scenes * horizon * sizeof(float)}, {blocked, s4}};
  for (int j = 0; j < 6; ++j)
    ADX_REQUIRE(ins[j].p == nullptr || !byte_ranges_overlap(state, metrics_state_bytes(), ins[j].p, ins[j].n),
                "metrics accumulate: the state overlaps an input");
  AccumulateArgs a;
  a.state = state; a.rec = rec; a.flags = flags; a.best = best; a.index = index; a.disp_sel = disp_sel; a.blocked = blocked;
  a.scenes = scenes; a.H = horizon;
  metrics_accumulate_kernel<<<dim3(1), dim3(256), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

}  // namespace adx
