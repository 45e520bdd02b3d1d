// The attention block of MODEL.USE_ATTN (modeling/helpers.py:120-175):  y = x + to_out(attn(LayerNorm(x)))  on x [B][C][L].
//
// to_qkv and to_out are ordinary 1x1 temporal convs (tconv_forward; to_out carries its bias and the residual x in the
// epilogue).  This file holds what sits between them, in plain fp32 FMAs -- the softmax and the LayerNorm statistics are
// the precision-sensitive part, and the work is small (C <= 512 per position, 32 x 32 x L per head):
//   chan_layernorm_fwd / _bwd   LayerNorm over channels per (sample, position): one wave each, biased variance, eps 1e-5,
//                               affine g, b
//   linattn_core_fwd / _bwd     per (sample, head): q *= 32^-0.5, k = softmax over positions, context = k v^T (32 x 32),
//                               out = context^T q; channel = head * 32 + c in each of q, k, v (einops "(h c)")
// A horizon that is not a power of two runs on the next one (adx_tconv_desc::lin_valid): the softmax and the context sum
// cover the L_valid real positions only, and padded outputs / gradients are written as 0.
#include "adx_common.h"

namespace adx {

constexpr int kHeads = 4, kHeadDim = 32, kHidden = kHeads * kHeadDim;   // LinearAttention(dim, heads=4, dim_head=32)
constexpr int kAttnMaxL = 64;                                           // padded length one workgroup holds in LDS
constexpr int kAttnPitch = kAttnMaxL + 1;

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// ---- LayerNorm over channels --------------------------------------------------------------------------------------------
// one wave per (sample, position), four per workgroup: the lanes split the channels and meet in wave reductions
__global__ void __launch_bounds__(256) chan_layernorm_fwd_kernel(const float* __restrict__ x, int64_t sb, int64_t sc, int64_t sl,
                                                                  const float* __restrict__ g, const float* __restrict__ bta,
                                                                  float* __restrict__ xn, float* __restrict__ mean_out,
                                                                  float* __restrict__ rstd_out, int B, int C, int L, int Lv) {
  const int idx = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (idx >= B * L) return;
  const int b = idx / L, l = idx - b * L;
  float* yo = xn + (int64_t)b * C * L + l;
  if (l >= Lv) {
    for (int c = lane; c < C; c += 64) yo[(int64_t)c * L] = 0.f;
    if (mean_out != nullptr && lane == 0) { mean_out[idx] = 0.f; rstd_out[idx] = 0.f; }
    return;
  }
  const float* xi = x + (int64_t)b * sb + (int64_t)l * sl;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += xi[(int64_t)c * sc];
  const float mean = wave_sum(s) / (float)C;
  float v = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float d = xi[(int64_t)c * sc] - mean;
    v = fmaf(d, d, v);
  }
  const float rstd = 1.f / sqrtf(wave_sum(v) / (float)C + 1e-5f);
  for (int c = lane; c < C; c += 64) yo[(int64_t)c * L] = (xi[(int64_t)c * sc] - mean) * rstd * g[c] + bta[c];
  if (mean_out != nullptr && lane == 0) { mean_out[idx] = mean; rstd_out[idx] = rstd; }
}

// dx = rstd * (dxh - mean_c(dxh) - xhat * mean_c(dxh * xhat)),  dxh = dy * g;  written, or added to dx (accumulate)
__global__ void __launch_bounds__(256) chan_layernorm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                  int64_t sb, int64_t sc, int64_t sl, const float* __restrict__ mean,
                                                                  const float* __restrict__ rstd, const float* __restrict__ g,
                                                                  float* __restrict__ dx, int B, int C, int L, int Lv, int accumulate) {
  const int idx = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (idx >= B * L) return;
  const int b = idx / L, l = idx - b * L;
  float* dxo = dx + (int64_t)b * C * L + l;
  if (l >= Lv) {
    if (!accumulate)
      for (int c = lane; c < C; c += 64) dxo[(int64_t)c * L] = 0.f;
    return;
  }
  const float* xi = x + (int64_t)b * sb + (int64_t)l * sl;
  const float* dyi = dy + (int64_t)b * C * L + l;
  const float mu = mean[idx], rs = rstd[idx];
  float s1 = 0.f, s2 = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float dxh = dyi[(int64_t)c * L] * g[c];
    s1 += dxh;
    s2 = fmaf(dxh, (xi[(int64_t)c * sc] - mu) * rs, s2);
  }
  s1 = wave_sum(s1) / (float)C;
  s2 = wave_sum(s2) / (float)C;
  for (int c = lane; c < C; c += 64) {
    const float xh = (xi[(int64_t)c * sc] - mu) * rs;
    const float v = rs * (dyi[(int64_t)c * L] * g[c] - s1 - xh * s2);
    dxo[(int64_t)c * L] = accumulate ? dxo[(int64_t)c * L] + v : v;
  }
}

// dg[c] = sum over (b, l < Lv) of dy * xhat, db[c] = sum of dy: one workgroup per channel, written (each LayerNorm owns its
// two tensors), reduced in a fixed order
__global__ void __launch_bounds__(256) chan_layernorm_affine_grad_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                         int64_t sb, int64_t sc, int64_t sl,
                                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                         float* __restrict__ dg, float* __restrict__ db, int B, int C,
                                                                         int L, int Lv) {
  const int c = blockIdx.x, tid = threadIdx.x;
  float sg = 0.f, sbb = 0.f;
  for (int i = tid; i < B * L; i += 256) {
    const int b = i / L, l = i - b * L;
    if (l >= Lv) continue;
    const float d = dy[((int64_t)b * C + c) * L + l];
    const float xh = (x[(int64_t)b * sb + (int64_t)c * sc + (int64_t)l * sl] - mean[i]) * rstd[i];
    sg = fmaf(d, xh, sg);
    sbb += d;
  }
  __shared__ float red[2][4];
  sg = wave_sum(sg);
  sbb = wave_sum(sbb);
  if ((tid & 63) == 0) { red[0][tid >> 6] = sg; red[1][tid >> 6] = sbb; }
  __syncthreads();
  if (tid == 0) {
    dg[c] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    db[c] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// ---- linear attention core: one workgroup (4 waves) per (sample, head) -------------------------------------------------------
// rows 0..31 of `dst` <- channel base + row of t[b] (zero past Lv), times `scale`
__device__ __forceinline__ void load_head(float (*dst)[kAttnPitch], const float* __restrict__ t, int64_t sb, int b, int ch0,
                                          int L, int Lv, float scale) {
  for (int i = threadIdx.x; i < kHeadDim * L; i += 256) {
    const int r = i / L, n = i - r * L;
    dst[r][n] = n < Lv ? t[(int64_t)b * sb + (int64_t)(ch0 + r) * L + n] * scale : 0.f;
  }
}

// k[d][n] <- softmax over n < Lv (zero past Lv); wave w owns rows 8w .. 8w + 7, lane = position
__device__ __forceinline__ void softmax_rows(float (*k)[kAttnPitch], int L, int Lv) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int r = w * 8; r < w * 8 + 8; ++r) {
    const bool live = lane < Lv;
    const float v = live ? k[r][lane] : -INFINITY;
    const float m = wave_max(v);
    const float e = live ? expf(v - m) : 0.f;
    const float sum = wave_sum(e);
    if (lane < L) k[r][lane] = e / sum;
  }
}

constexpr float kQScale = 0.17677669529663687f;   // 32 ** -0.5

__global__ void __launch_bounds__(256) linattn_core_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ o, int L, int Lv) {
  __shared__ float q[kHeadDim][kAttnPitch], k[kHeadDim][kAttnPitch], v[kHeadDim][kAttnPitch];
  __shared__ float ctx[kHeadDim][kHeadDim + 1];
  const int b = blockIdx.x / kHeads, h = blockIdx.x % kHeads, tid = threadIdx.x;
  const int64_t sb = (int64_t)3 * kHidden * L;
  load_head(q, qkv, sb, b, h * kHeadDim, L, Lv, kQScale);
  load_head(k, qkv, sb, b, kHidden + h * kHeadDim, L, Lv, 1.f);
  load_head(v, qkv, sb, b, 2 * kHidden + h * kHeadDim, L, Lv, 1.f);
  __syncthreads();
  softmax_rows(k, L, Lv);
  __syncthreads();
  for (int i = tid; i < kHeadDim * kHeadDim; i += 256) {    // context[d][e] = sum_n k[d][n] v[e][n]
    const int d = i / kHeadDim, e = i % kHeadDim;
    float s = 0.f;
    for (int n = 0; n < Lv; ++n) s = fmaf(k[d][n], v[e][n], s);
    ctx[d][e] = s;
  }
  __syncthreads();
  float* ob = o + (int64_t)b * kHidden * L + (int64_t)h * kHeadDim * L;
  for (int i = tid; i < kHeadDim * L; i += 256) {            // out[e][n] = sum_d context[d][e] q[d][n]
    const int e = i / L, n = i - e * L;
    float s = 0.f;
    for (int d = 0; d < kHeadDim; ++d) s = fmaf(ctx[d][e], q[d][n], s);
    ob[(int64_t)e * L + n] = n < Lv ? s : 0.f;
  }
}

// dO [B][128][L] -> dqkv [B][384][L] (written).  With q' = q * s, ks = softmax(k):
//   dctx[d][e] = sum_n q'[d][n] dO[e][n]          dq[d][n]  = s * sum_e ctx[d][e] dO[e][n]
//   dv[e][n]   = sum_d dctx[d][e] ks[d][n]        dks[d][n] = sum_e dctx[d][e] v[e][n]
//   dk[d][n]   = ks[d][n] (dks[d][n] - sum_m ks[d][m] dks[d][m])
__global__ void __launch_bounds__(256) linattn_core_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                               float* __restrict__ dqkv, int L, int Lv) {
  __shared__ float q[kHeadDim][kAttnPitch], k[kHeadDim][kAttnPitch], v[kHeadDim][kAttnPitch], go[kHeadDim][kAttnPitch];
  __shared__ float ctx[kHeadDim][kHeadDim + 1], dctx[kHeadDim][kHeadDim + 1];
  const int b = blockIdx.x / kHeads, h = blockIdx.x % kHeads, tid = threadIdx.x;
  const int64_t sb = (int64_t)3 * kHidden * L;
  load_head(q, qkv, sb, b, h * kHeadDim, L, Lv, kQScale);
  load_head(k, qkv, sb, b, kHidden + h * kHeadDim, L, Lv, 1.f);
  load_head(v, qkv, sb, b, 2 * kHidden + h * kHeadDim, L, Lv, 1.f);
  load_head(go, dout, (int64_t)kHidden * L, b, h * kHeadDim, L, Lv, 1.f);
  __syncthreads();
  softmax_rows(k, L, Lv);
  __syncthreads();
  for (int i = tid; i < kHeadDim * kHeadDim; i += 256) {
    const int d = i / kHeadDim, e = i % kHeadDim;
    float s = 0.f, t = 0.f;
    for (int n = 0; n < Lv; ++n) {
      s = fmaf(k[d][n], v[e][n], s);
      t = fmaf(q[d][n], go[e][n], t);
    }
    ctx[d][e] = s;
    dctx[d][e] = t;
  }
  __syncthreads();            // q is dead from here: it receives dks
  float* gb = dqkv + (int64_t)b * 3 * kHidden * L;
  for (int i = tid; i < kHeadDim * L; i += 256) {
    const int r = i / L, n = i - r * L;
    float dq = 0.f, dv = 0.f, dks = 0.f;
    for (int j = 0; j < kHeadDim; ++j) {
      dq = fmaf(ctx[r][j], go[j][n], dq);
      dv = fmaf(dctx[j][r], k[j][n], dv);
      dks = fmaf(dctx[r][j], v[j][n], dks);
    }
    const bool live = n < Lv;
    gb[(int64_t)(h * kHeadDim + r) * L + n] = live ? dq * kQScale : 0.f;
    gb[(int64_t)(2 * kHidden + h * kHeadDim + r) * L + n] = live ? dv : 0.f;
    q[r][n] = live ? dks : 0.f;
  }
  __syncthreads();
  const int w = tid >> 6, lane = tid & 63;
  for (int r = w * 8; r < w * 8 + 8; ++r) {
    const bool live = lane < Lv;
    const float ks = live ? k[r][lane] : 0.f, dks = live ? q[r][lane] : 0.f;
    const float dot = wave_sum(ks * dks);
    if (lane < L) gb[(int64_t)(kHidden + h * kHeadDim + r) * L + lane] = live ? ks * (dks - dot) : 0.f;
  }
}

static int attn_check_len(int L, int Lv, const char* who) {
  ADX_REQUIRE(L >= 1 && L <= kAttnMaxL && Lv >= 1 && Lv <= L, "%s: length %d (valid %d) outside 1..%d", who, L, Lv, kAttnMaxL);
  return ADX_OK;
}

int chan_layernorm_forward(const float* x, int64_t sb, int64_t sc, int64_t sl, const float* g, const float* b, float* xn,
                           float* mean, float* rstd, int B, int C, int L, int L_valid, hipStream_t s) {
  const int Lv = L_valid > 0 ? L_valid : L;
  ADX_REQUIRE(x && g && b && xn && B >= 1 && C >= 1 && L >= 1 && Lv <= L && (mean == nullptr) == (rstd == nullptr),
              "chan_layernorm_forward: bad argument");
  if (PlanSink* ps = plan_sink()) {      // the plan export (plan.h): record, do not launch
    PlanLaunch l;
    l.aux = 3; l.rows = B; l.grid = ceil_div(B * L, 4);
    return plan_emit(ps, l);
  }
  chan_layernorm_fwd_kernel<<<dim3(ceil_div(B * L, 4)), dim3(256), 0, s>>>(x, sb, sc, sl, g, b, xn, mean, rstd, B, C, L, Lv);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

int chan_layernorm_backward(const float* dy, const float* x, int64_t sb, int64_t sc, int64_t sl, const float* mean,
                            const float* rstd, const float* g, float* dx, float* dg, float* db, int B, int C, int L, int L_valid,
                            bool accumulate, hipStream_t s) {
  const int Lv = L_valid > 0 ? L_valid : L;
  ADX_REQUIRE(dy && x && mean && rstd && g && dx && dg && db && B >= 1 && C >= 1 && L >= 1 && Lv <= L,
              "chan_layernorm_backward: bad argument");
  chan_layernorm_bwd_kernel<<<dim3(ceil_div(B * L, 4)), dim3(256), 0, s>>>(dy, x, sb, sc, sl, mean, rstd, g, dx, B, C, L, Lv,
                                                                           accumulate ? 1 : 0);
  ADX_LAUNCH_CHECK();
  chan_layernorm_affine_grad_kernel<<<dim3(C), dim3(256), 0, s>>>(dy, x, sb, sc, sl, mean, rstd, dg, db, B, C, L, Lv);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

int linattn_core_forward(const float* qkv, float* o, int B, int L, int L_valid, hipStream_t s) {
  const int Lv = L_valid > 0 ? L_valid : L;
  ADX_REQUIRE(qkv && o && B >= 1, "linattn_core_forward: bad argument");
  const int rc = attn_check_len(L, Lv, "linattn_core_forward");
  if (rc != ADX_OK) return rc;
  if (PlanSink* ps = plan_sink()) {      // the plan export (plan.h): record, do not launch
    PlanLaunch l;
    l.aux = 4; l.rows = B; l.grid = B * kHeads;
    return plan_emit(ps, l);
  }
  linattn_core_fwd_kernel<<<dim3(B * kHeads), dim3(256), 0, s>>>(qkv, o, L, Lv);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

int linattn_core_backward(const float* qkv, const float* dout, float* dqkv, int B, int L, int L_valid, hipStream_t s) {
  const int Lv = L_valid > 0 ? L_valid : L;
  ADX_REQUIRE(qkv && dout && dqkv && B >= 1, "linattn_core_backward: bad argument");
  const int rc = attn_check_len(L, Lv, "linattn_core_backward");
  if (rc != ADX_OK) return rc;
  linattn_core_bwd_kernel<<<dim3(B * kHeads), dim3(256), 0, s>>>(qkv, dout, dqkv, L, Lv);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

}  // namespace adx

extern "C" {

int adx_chan_layernorm_forward(const float* x, int64_t sb, int64_t sc, int64_t sl, const float* g, const float* b, float* xn,
                               float* mean, float* rstd, int32_t B, int32_t C, int32_t L, int32_t L_valid, adx_stream s) {
  return adx::chan_layernorm_forward(x, sb, sc, sl, g, b, xn, mean, rstd, B, C, L, L_valid, (hipStream_t)s);
}

int adx_chan_layernorm_backward(const float* dy, const float* x, int64_t sb, int64_t sc, int64_t sl, const float* mean,
                                const float* rstd, const float* g, float* dx, float* dg, float* db, int32_t B, int32_t C,
                                int32_t L, int32_t L_valid, int32_t accumulate, adx_stream s) {
  return adx::chan_layernorm_backward(dy, x, sb, sc, sl, mean, rstd, g, dx, dg, db, B, C, L, L_valid, accumulate != 0,
                                      (hipStream_t)s);
}

int adx_linattn_forward(const float* qkv, float* o, int32_t B, int32_t L, int32_t L_valid, adx_stream s) {
  return adx::linattn_core_forward(qkv, o, B, L, L_valid, (hipStream_t)s);
}

int adx_linattn_backward(const float* qkv, const float* dout, float* dqkv, int32_t B, int32_t L, int32_t L_valid, adx_stream s) {
  return adx::linattn_core_backward(qkv, dout, dqkv, B, L, L_valid, (hipStream_t)s);
}

}  // extern "C"
