// Manoeuvre commitment (include/adx.h: adx_traj_commit, "manoeuvre commitment v1"): hold the previous tick's manoeuvre unless the
// selector's new choice is clearly better.  No reference counterpart: the reference samples one trajectory per tick
// (interact.py:110-140) and has nothing to commit to.
//
// One workgroup per scene, 256 threads = 4 waves, as modes.hip: the work is K * n distance terms against ONE polyline, and the
// candidates of a scene lie S rows apart in memory (candidate-major), so a lane that walked its own candidate in global memory
// would fetch one 4-byte word per 64-byte line and waypoint.  Instead all 256 threads stage the scored xy in LDS as two planes
// with a candidate stride of 65 words (odd: the 32 lanes of each half wave fall on 32 different banks), and the decision is one
// wave's work:
//   0. every thread reads the scene's `valid` and `held` words; the first wave (lane = waypoint) forms the prior q_h from the
//      stored plan -- warm start v1's advance (warm_advance of sched.h, shared with warm_init_kernel) and re-base, cosf / sinf once
//      in lane 0 and broadcast -- into LDS.  Nothing of the scene's state is written before the barrier that ends phase 2;
//   1. the staging above;
//   2. the first wave, lane = candidate: d_k by the h-sequential sum, one ballot each for finite, near and eligible, a xor
//      butterfly over (cost, index) for the follower, the decision of the contract's table in every lane alike, and lane 0 writes
//      index, status, follower and blocked;
//   3. all threads copy the chosen row word for word and write the next state.
// No atomics and no inter-workgroup traffic: a given input and state give the same bits on every launch.
#include "sched.h"

namespace adx {

namespace {

constexpr int kComMaxK = 64, kComMaxH = 64, kComMaxD = 16;
constexpr int kComStride = kComMaxH + 1;      // odd: lanes holding different candidates hit different banks
constexpr int kNoPrior = 0, kSame = 1, kLost = 2, kHeld = 3, kSwitched = 4;

struct CommitArgs {
  const float* trajs;
  const float* cost;          // [scenes][K]
  const int32_t* selected;    // [scenes]
  const int32_t* active;      // [scenes][K] or null
  const float* motion;        // [scenes][3] or null
  uint32_t* state;            // [scenes][2 + 2H]
  float* best;                // [scenes][H][D]
  int32_t* index;             // [scenes]
  int32_t* status;            // [scenes]
  int32_t* follower;          // [scenes]
  int32_t* blocked;           // [scenes] or null
  float* dist2;               // [scenes][K]
  int scenes, K, H, D, h0, shift, max_hold;
  float r2, margin, ratio;
};

__global__ void __launch_bounds__(256) traj_commit_kernel(const CommitArgs a) {
#pragma clang fp contract(off)
  __shared__ float xs[kComMaxK * kComStride], ys[kComMaxK * kComStride];
  __shared__ float qx_s[kComMaxH], qy_s[kComMaxH];
  __shared__ int chosen_s, status_s, finite_s;
  const int s = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int K = a.K, H = a.H, D = a.D, h0 = a.h0;
  const int n = H - h0;
  const size_t row_floats = (size_t)H * D;
  uint32_t* st = a.state + (size_t)s * (2 + 2 * H);

  // 0. the state, read before anything of the scene is written
  const int valid = (int)st[0], held = (int)st[1];
  if (wave == 0) {
    const float* p = reinterpret_cast<const float*>(st + 2);      // the stored plan, [H][2]
    float c = 0.f, sn = 0.f, tx = 0.f, ty = 0.f;
    if (a.motion != nullptr) {
      if (lane == 0) {
        const float phi = a.motion[(size_t)s * 3 + 2];
        c = cosf(phi);
        sn = sinf(phi);
      }
      c = __shfl(c, 0, 64);
      sn = __shfl(sn, 0, 64);
      tx = a.motion[(size_t)s * 3 + 0];
      ty = a.motion[(size_t)s * 3 + 1];
    }
    if (lane < H) {
      const float ux = warm_advance(p, lane, 0, H, 2, a.shift), uy = warm_advance(p, lane, 1, H, 2, a.shift);
      float wx, wy;
      if (a.motion != nullptr) {
        const float qx = ux - tx, qy = uy - ty;
        const float m0 = c * qx, m1 = sn * qy;
        wx = m0 + m1;
        const float n0 = sn * qx, n1 = c * qy;
        wy = -n0 + n1;
      } else {
        wx = ux - p[a.shift * 2 + 0];
        wy = uy - p[a.shift * 2 + 1];
      }
      qx_s[lane] = wx;
      qy_s[lane] = wy;
    }
  }

  // 1. stage the scored waypoints: element i = k * n + (h - h0) of the scene; candidate k of scene s is row k * scenes + s
  for (int i = tid; i < K * n; i += 256) {
    const int k = i / n, hh = i - k * n;
    const float* p = a.trajs + ((size_t)k * a.scenes + s) * row_floats + (size_t)(h0 + hh) * D;
    xs[k * kComStride + hh] = p[0];
    ys[k * kComStride + hh] = D > 1 ? p[1] : 0.f;
  }
  __syncthreads();

  // 2. the decision: lane = candidate
  if (wave == 0) {
    const bool in = lane < K;
    const int own = lane * kComStride;      // lanes >= K never read
    const bool q_bad = lane < n && !(finite_f(qx_s[h0 + lane]) && finite_f(qy_s[h0 + lane]));
    const bool prior = valid != 0 && __ballot(q_bad) == 0ull;
    bool fin = in;
    float d = 0.f;
    if (in) {
      float acc = 0.f;
      for (int hh = 0; hh < n; ++hh) {
        const float x = xs[own + hh], y = ys[own + hh];
        fin = fin && finite_f(x) && finite_f(y);
        const float dx = x - qx_s[h0 + hh], dy = y - qy_s[h0 + hh];
        acc = acc + (dx * dx + dy * dy);
      }
      d = acc / (float)n;
      a.dist2[(size_t)s * K + lane] = d;
    }
    const unsigned long long finite = __ballot(fin);
    const bool near = fin && d <= a.r2;
    const unsigned long long near_m = __ballot(near);
    int sel = a.selected[s];
    sel = sel < 0 ? 0 : (sel > K - 1 ? K - 1 : sel);      // the contract: clamped into range
    const float ck = in ? a.cost[(size_t)s * K + lane] : __builtin_inff();
    const int act = (in && a.active != nullptr) ? a.active[(size_t)s * K + lane] : 0;
    const float cost_sel = __shfl(ck, sel, 64);
    const int act_sel = __shfl(act, sel, 64);
    const bool elig = near && finite_f(ck) && (act == 0 || act_sel != 0);
    const unsigned long long elig_m = __ballot(elig);
    float v = elig ? ck : __builtin_inff();
    int idx = lane;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(v, off, 64);
      const int oi = __shfl_xor(idx, off, 64);
      if (ov < v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
    const float t0 = cost_sel + a.margin, t1 = a.ratio * __builtin_fabsf(cost_sel);
    const float t = t0 + t1;
    int status, chosen = sel, f = -1;
    if (!prior) {
      status = kNoPrior;
    } else if (((near_m >> sel) & 1ull) != 0ull) {
      status = kSame;
    } else if (elig_m == 0ull) {
      status = kLost;
    } else {
      f = idx;      // an eligible lane: its cost is finite, so v is
      if (v <= t && (a.max_hold == 0 || held < a.max_hold)) {
        status = kHeld;
        chosen = f;
      } else {
        status = kSwitched;
      }
    }
    const int act_chosen = __shfl(act, chosen, 64);
    if (lane == 0) {
      a.index[s] = chosen;
      a.status[s] = status;
      a.follower[s] = f;
      if (a.blocked != nullptr && a.active != nullptr) a.blocked[s] = act_chosen != 0 ? 1 : 0;
      chosen_s = chosen;
      status_s = status;
      finite_s = (int)((finite >> chosen) & 1ull);
    }
  }
  __syncthreads();

  // 3. the chosen row, bit for bit, and the next state.  An unfinite choice leaves the stored plan as it is under valid = 0
  const int chosen = chosen_s;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.trajs + ((size_t)chosen * a.scenes + s) * row_floats);
  uint32_t* dst = reinterpret_cast<uint32_t*>(a.best + (size_t)s * row_floats);
  const int words = H * D;
  for (int i = tid; i < words; i += 256) dst[i] = src[i];
  if (tid == 0) {
    st[0] = finite_s != 0 ? 1u : 0u;
    st[1] = status_s == kHeld ? (uint32_t)(held + 1) : 0u;
  }
  if (finite_s != 0 && tid < H) {
    st[2 + 2 * tid] = src[tid * D];
    st[3 + 2 * tid] = D > 1 ? src[tid * D + 1] : 0u;
  }
}

__global__ void __launch_bounds__(256) commit_reset_kernel(uint32_t* state, const uint8_t* mask, int scenes, int stride) {
  const int i = blockIdx.x * 256 + threadIdx.x;        // scenes * stride <= 65535 * 130: fits
  if (i >= scenes * stride) return;
  if (mask == nullptr || mask[i / stride] != 0) state[i] = 0u;
}

bool commit_shape_ok(int scenes, int horizon) { return scenes >= 1 && scenes <= 65535 && horizon >= 2 && horizon <= kComMaxH; }

}  // namespace

size_t commit_state_bytes(int scenes, int horizon) {
  return commit_shape_ok(scenes, horizon) ? (size_t)scenes * (2 + 2 * horizon) * sizeof(uint32_t) : 0;
}

int commit_reset(void* state, int scenes, int horizon, const uint8_t* mask, hipStream_t s) {
  ADX_REQUIRE(scenes >= 1 && scenes <= 65535, "commit reset: %d scenes, supported 1..65535", scenes);
  ADX_REQUIRE(horizon >= 2 && horizon <= kComMaxH, "commit reset: horizon %d, supported 2..%d", horizon, kComMaxH);
  ADX_REQUIRE(state != nullptr, "commit reset: null state");
  const int stride = 2 + 2 * horizon;
  ADX_REQUIRE(mask == nullptr || !byte_ranges_overlap(state, (size_t)scenes * stride * sizeof(uint32_t), mask, (size_t)scenes),
              "commit reset: the mask overlaps the state");
  commit_reset_kernel<<<dim3(ceil_div(scenes * stride, 256)), dim3(256), 0, s>>>(static_cast<uint32_t*>(state), mask, scenes, stride);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

int traj_commit(const adx_commit_cfg* c, const float* trajs, const float* cost, const int32_t* selected, const int32_t* active,
                const float* motion, void* state, float* best, int32_t* index, int32_t* status, int32_t* follower, int32_t* blocked,
                float* dist2, hipStream_t s) {
  ADX_REQUIRE(c != nullptr, "traj commit: null configuration");
  const int S = c->scenes, K = c->candidates, H = c->horizon, D = c->dim;
  ADX_REQUIRE(K >= 1 && K <= kComMaxK, "traj commit: %d candidates, supported 1..%d", K, kComMaxK);
  ADX_REQUIRE(H >= 2 && H <= kComMaxH, "traj commit: horizon %d, supported 2..%d", H, kComMaxH);
  ADX_REQUIRE(D >= 1 && D <= kComMaxD, "traj commit: transition dim %d, supported 1..%d", D, kComMaxD);
  ADX_REQUIRE(S >= 1 && S <= 65535, "traj commit: %d scenes, supported 1..65535", S);
  ADX_REQUIRE(c->h0 >= 0 && c->h0 <= H - 1, "traj commit: h0 %d, supported 0..%d (horizon - 1)", c->h0, H - 1);
  ADX_REQUIRE(c->shift >= 0 && c->shift <= H - 1, "traj commit: shift %d, supported 0..%d (horizon - 1)", c->shift, H - 1);
  ADX_REQUIRE(c->max_hold >= 0, "traj commit: max_hold %d must be >= 0", c->max_hold);
  ADX_REQUIRE(finite_f(c->radius) && c->radius >= 0.f, "traj commit: radius %g must be finite and >= 0", (double)c->radius);
  ADX_REQUIRE(finite_f(c->margin) && c->margin >= 0.f, "traj commit: margin %g must be finite and >= 0", (double)c->margin);
  ADX_REQUIRE(finite_f(c->ratio) && c->ratio >= 0.f, "traj commit: ratio %g must be finite and >= 0", (double)c->ratio);
  ADX_REQUIRE(trajs != nullptr, "traj commit: null trajs");
  ADX_REQUIRE(cost != nullptr, "traj commit: null cost");
  ADX_REQUIRE(selected != nullptr, "traj commit: null selected");
  ADX_REQUIRE(state != nullptr, "traj commit: null state");
  ADX_REQUIRE(best != nullptr, "traj commit: null best");
  ADX_REQUIRE(index != nullptr, "traj commit: null index");
  ADX_REQUIRE(status != nullptr, "traj commit: null status");
  ADX_REQUIRE(follower != nullptr, "traj commit: null follower");
  ADX_REQUIRE(dist2 != nullptr, "traj commit: null dist2");
  ADX_REQUIRE(blocked == nullptr || active != nullptr, "traj commit: blocked given without active");
  const size_t row = (size_t)H * D * sizeof(float);
  const ByteSpan ins[6] = {{trajs, (size_t)K * S * row},
                           {cost, (size_t)S * K * sizeof(float)},
                           {selected, (size_t)S * sizeof(int32_t)},
                           {active, (size_t)S * K * sizeof(int32_t)},
                           {motion, (size_t)S * 3 * sizeof(float)},
                           {state, commit_state_bytes(S, H)}};
  const char* const in_names[6] = {"trajs", "cost", "selected", "active", "motion", "the state"};
  const ByteSpan outs[6] = {{best, (size_t)S * row},
                            {index, (size_t)S * sizeof(int32_t)},
                            {status, (size_t)S * sizeof(int32_t)},
                            {follower, (size_t)S * sizeof(int32_t)},
                            {blocked, (size_t)S * sizeof(int32_t)},
                            {dist2, (size_t)S * K * sizeof(float)}};
  const char* const names[6] = {"best", "index", "status", "follower", "blocked", "dist2"};
  for (int i = 0; i < 6; ++i) {
    if (outs[i].p == nullptr) continue;      // blocked alone may be
    for (int j = 0; j < 6; ++j)
      ADX_REQUIRE(ins[j].p == nullptr || !byte_ranges_overlap(outs[i].p, outs[i].n, ins[j].p, ins[j].n), "traj commit: %s aliases %s",
                  names[i], in_names[j]);
    for (int j = 0; j < i; ++j)
      ADX_REQUIRE(outs[j].p == nullptr || !byte_ranges_overlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n),
                  "traj commit: %s and %s alias each other", names[j], names[i]);
  }
  for (int j = 0; j < 5; ++j)
    ADX_REQUIRE(ins[j].p == nullptr || !byte_ranges_overlap(ins[5].p, ins[5].n, ins[j].p, ins[j].n), "traj commit: the state aliases %s",
                in_names[j]);
  CommitArgs a = {};
  a.trajs = trajs; a.cost = cost; a.selected = selected; a.active = active; a.motion = motion;
  a.state = static_cast<uint32_t*>(state);
  a.best = best; a.index = index; a.status = status; a.follower = follower; a.blocked = blocked; a.dist2 = dist2;
  a.scenes = S; a.K = K; a.H = H; a.D = D; a.h0 = c->h0; a.shift = c->shift; a.max_hold = c->max_hold;
  a.r2 = c->radius * c->radius;      // rounded once
  a.margin = c->margin; a.ratio = c->ratio;
  traj_commit_kernel<<<dim3(S), dim3(256), 0, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

}  // namespace adx
