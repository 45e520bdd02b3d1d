// ResNet-34 perception forward (eval mode) on the fp32 matrix cores of gfx950.
//   modeling/resnet.py:56-102 (BasicBlock), :163-296 (ResNet), fc replaced by Linear(512, dim)
//   at modeling/temporal.py:83-84.  This is 99.5 % of the FLOPs of one reference forward
//   (34 GFLOP per 3x256x900 image).
//
// conv2d = implicit GEMM, C[cout][pixel] = sum_k W[cout][k] * X[k][pixel], k = (tap, cin):
//   * v_mfma_f32_32x32x2_f32: A = weights (32 couts x 2 k), B = activations (2 k x 32 pixels),
//     so a lane of the accumulator owns one pixel column -> NCHW stores are 128-byte rows and
//     the tensors keep PyTorch's layout end to end (no layout conversion of the camera image);
//   * one workgroup = 4 waves = 4 output rows x 32 output columns x 64 output channels; per
//     16-channel chunk the zero-padded input patch and the [tap][cin][64] weight slab are staged
//     in LDS (both read conflict-free: consecutive lanes = consecutive columns / channels);
//   * epilogue fuses eval-mode BatchNorm as y = acc * scale[c] + shift[c] (the same
//     alpha/beta form torch uses), the residual add and ReLU.
#include <stdlib.h>

#include <vector>

#include "adx_common.h"
#include "conv2d_internal.h"

namespace adx {

constexpr int kCoutT = 64;   // output channels per workgroup (2 MFMA row blocks)
constexpr size_t kMaxLds = 96 * 1024;

// Software pipeline (register double buffer): the global loads of chunk i+1 (input patch + weight
// slab) are issued before the MFMAs of chunk i and written to LDS after them, so HBM/L2 latency
// hides behind ~9k cycles of matrix work per 16-channel chunk.
// ROWS = output rows per wave (tile = 4*ROWS rows x 32 columns x 64 channels): ROWS = 2 reuses every
// weight fragment for two pixel rows (1.0 instead of 1.5 LDS reads per MFMA).
template <int STRIDE, int K, int ROWS, int CCH = 16>
__global__ void __launch_bounds__(256) conv2d_kernel(const Conv2dArgs a) {
  constexpr int TH = 4 * ROWS;
  constexpr int CC = (K == 7) ? 4 : CCH;                  // channels per chunk
  constexpr int PH = (TH - 1) * STRIDE + K;           // staged patch rows / columns
  constexpr int PW = (kTileW - 1) * STRIDE + K;
  constexpr int PLANE = PH * PW;
  constexpr int NP = CC * PLANE;                          // patch floats per chunk
  constexpr int PITEMS = (NP + 255) / 256;
  constexpr int NTAPS = K * K;
  constexpr int NW4 = NTAPS * CC * (kCoutT / 4);          // weight float4s per chunk
  constexpr int WITEMS = (NW4 + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* patch = smem;                                    // [CC][PH][PW]
  float* wl = smem + PITEMS * 256;                        // [NTAPS][CC][64]
  float* ss = wl + NTAPS * CC * kCoutT;                   // scale[64], shift[64]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bid = blockIdx.x;
  const int ct = bid % a.cout_tiles; bid /= a.cout_tiles;
  const int tx = bid % a.tiles_x; bid /= a.tiles_x;
  const int ty = bid % a.tiles_y; bid /= a.tiles_y;
  const int n = bid;
  const int oy0 = ty * TH, ox0 = tx * kTileW;
  const int iy0 = oy0 * STRIDE - a.pad, ix0 = ox0 * STRIDE - a.pad;
  const int cout0 = ct * kCoutT;
  const int l31 = lane & 31, khalf = lane >> 5;
  const size_t hw = (size_t)a.H * a.W;
  const float* xin = a.x + (size_t)n * a.Cin * hw;

  // per-thread gather offsets of its patch elements, identical for every chunk (-1 = zero padding)
  int goff[PITEMS];
#pragma unroll
  for (int k = 0; k < PITEMS; ++k) {
    const int e = tid + 256 * k;
    const int c = e / PLANE, rem = e - c * PLANE;
    const int py = rem / PW, px = rem - py * PW;
    const int iy = iy0 + py, ix = ix0 + px;
    const bool ok = e < NP && c < a.Cin && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
    goff[k] = ok ? (int)(c * hw + (size_t)iy * a.W + ix) : -1;
  }
  if (tid < 2 * kCoutT) {
    const int c = cout0 + (tid & (kCoutT - 1));
    ss[tid] = a.scale == nullptr ? (tid < kCoutT ? 1.f : 0.f) : (tid < kCoutT ? a.scale[c] : a.shift[c]);
  }

  f32x16 acc[ROWS][2];
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[r][0][i] = 0.f; acc[r][1][i] = 0.f; }
  float pv[PITEMS];
  f32x4 wv[WITEMS];
  auto load_chunk = [&](int c0) {
    const float* xc = xin + (size_t)c0 * hw;
#pragma unroll
    for (int k = 0; k < PITEMS; ++k) {
      const float v = xc[goff[k] >= 0 ? goff[k] : 0];   // branch-free: out-of-image taps read element 0 and are zeroed
      pv[k] = goff[k] >= 0 ? v : 0.f;
    }
#pragma unroll
    for (int k = 0; k < WITEMS; ++k) {
      const int e = tid + 256 * k;
      const int q = e & 15, row = e >> 4;             // row = tap * CC + c
      const int tap = row / CC, c = row - tap * CC;
      const int ec = e < NW4 ? e : 0;                    // clamp instead of branching; the store below is predicated
      const int rowc = ec >> 4, tapc = rowc / CC, cc_ = rowc - tapc * CC;
      (void)tap; (void)c;
      wv[k] = *reinterpret_cast<const f32x4*>(a.w + ((size_t)tapc * a.cin_pad + c0 + cc_) * a.Cout + cout0 + 4 * q);
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int k = 0; k < PITEMS; ++k) patch[tid + 256 * k] = pv[k];   // the patch area is padded to PITEMS * 256 floats
#pragma unroll
    for (int k = 0; k < WITEMS; ++k) {
      const int e = tid + 256 * k;
      if (e < NW4) *reinterpret_cast<f32x4*>(wl + 4 * e) = wv[k];
    }
  };

  load_chunk(0);
  for (int c0 = 0; c0 < a.cin_pad; c0 += CC) {
    if (c0 > 0) __syncthreads();          // everyone finished reading the previous chunk
    store_chunk();
    __syncthreads();
    if (c0 + CC < a.cin_pad) load_chunk(c0 + CC);   // in flight during the MFMAs below
#pragma unroll 1
    for (int kh = 0; kh < K; ++kh) {
#pragma unroll 1
      for (int kw = 0; kw < K; ++kw) {
        const float* pb = patch + (wave * ROWS * STRIDE + kh) * PW + l31 * STRIDE + kw + khalf * PLANE;
        const float* wa = wl + ((kh * K + kw) * CC + khalf) * kCoutT + l31;
#pragma unroll
        for (int ks = 0; ks < CC / 2; ++ks) {
          const float a0 = wa[2 * ks * kCoutT];
          const float a1 = wa[2 * ks * kCoutT + 32];
#pragma unroll
          for (int r = 0; r < ROWS; ++r) {
            const float b = pb[2 * ks * PLANE + r * STRIDE * PW];
            acc[r][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[r][0], 0, 0, 0);
            acc[r][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc[r][1], 0, 0, 0);
          }
        }
      }
    }
  }

  // ---- epilogue: BN scale/shift, residual, ReLU; lane = pixel column, register = channel --------
  const int ox = ox0 + l31;
  const size_t img = (size_t)n * a.Cout * a.OH * a.OW;
  const size_t plane_o = (size_t)a.OH * a.OW;
#pragma unroll
  for (int rr = 0; rr < ROWS; ++rr) {
    const int oy = oy0 + wave * ROWS + rr;
    if (oy >= a.OH || ox >= a.OW) continue;
    const size_t pix = (size_t)oy * a.OW + ox;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      float rv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cl = half * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
        rv[r] = a.res != nullptr ? a.res[img + (size_t)(cout0 + cl) * plane_o + pix] : 0.f;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cl = half * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
        float v = acc[rr][half][r];
        v = v * ss[cl] + ss[kCoutT + cl];
        v += rv[r];
        if (a.relu) v = v > 0.f ? v : 0.f;
        a.y[img + (size_t)(cout0 + cl) * plane_o + pix] = v;
      }
    }
  }
}

// [Cout][Cin][KH][KW] -> [KH*KW][cin_pad][Cout]
__global__ void conv2d_pack_kernel(const float* __restrict__ w, float* __restrict__ p, int Cout, int Cin, int taps,
                                   int cin_pad, size_t total) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int co = idx % Cout;
  const int ci = (idx / Cout) % cin_pad;
  const int tap = idx / ((size_t)Cout * cin_pad);
  p[idx] = ci < Cin ? w[((size_t)co * Cin + ci) * taps + tap] : 0.f;
}

// data-gradient image of the same weight: K = original cout, N = original cin, taps flipped:
// p[tap'][co][ci] = w[co][ci][taps-1-tap']
__global__ void conv2d_pack_dgrad_kernel(const float* __restrict__ w, float* __restrict__ p, int Cout, int Cin, int taps,
                                         size_t total) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int ci = idx % Cin;
  const int co = (idx / Cin) % Cout;
  const int tap = idx / ((size_t)Cin * Cout);
  p[idx] = w[((size_t)co * Cin + ci) * taps + (taps - 1 - tap)];
}

int conv2d_pack_spec(const ConvSpec& c, const float* w, float* packed, int dgrad, hipStream_t s) {
  if (conv2d_hs_eligible(c)) return conv2d_hs_pack(c, w, packed, dgrad, s);
  // dgrad: the forward weight is [c.cin][c.cout][k][k]
  return dgrad ? conv2d_pack_raw(w, packed, c.cin, c.cout, c.k, c.cin, 1, s)
               : conv2d_pack_raw(w, packed, c.cout, c.cin, c.k, c.cin_pad, 0, s);
}

int conv2d_pack_raw(const float* w, float* packed, int cout, int cin, int k, int cin_pad, int dgrad, hipStream_t s) {
  if (dgrad) {
    const size_t total = (size_t)k * k * cout * cin;
    conv2d_pack_dgrad_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s>>>(w, packed, cout, cin, k * k, total);
  } else {
    const size_t total = (size_t)k * k * cin_pad * cout;
    conv2d_pack_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s>>>(w, packed, cout, cin, k * k, cin_pad, total);
  }
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

// eval-mode BatchNorm2d as y = x * scale + shift (eps = 1e-5)
__global__ void bn_fold_kernel(const float* g, const float* b, const float* mean, const float* var, float* scale,
                               float* shift, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float s = g[c] / sqrtf(var[c] + 1e-5f);
  scale[c] = s;
  shift[c] = b[c] - mean[c] * s;
}

// MaxPool2d(kernel 3, stride 2, padding 1), modeling/resnet.py:197.  One wave per output row (blockIdx.x = plane),
// lanes along the row.  Even widths: a lane loads columns (2 ox, 2 ox + 1) as one 8-byte word -- every load
// instruction of a wave covers one contiguous 512-byte span, each input row is fetched exactly once -- and takes
// column 2 ox - 1 from its left neighbour's word (only the first lane of a 64-column chunk loads it itself).
__device__ __forceinline__ float pool_max(float m, float v) { return (v > m || v != v) ? v : m; }   // NaN propagates like torch

__global__ void __launch_bounds__(256) maxpool_kernel(const float* __restrict__ x, float* __restrict__ y, int planes,
                                                       int H, int W, int OH, int OW) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int oy = blockIdx.y * 4 + wave;
  const int pl = blockIdx.x;
  if (oy >= OH) return;
  const float* src = x + (size_t)pl * H * W;
  float* dst = y + ((size_t)pl * OH + oy) * OW;
  if ((W & 1) == 0 && ((size_t)x & 7) == 0) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    for (int ox0 = lane; ox0 - lane < OW; ox0 += 256) {   // wave-uniform trip count: the shuffles need every lane
      float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        const int iy = oy * 2 - 1 + dy;
        if (iy < 0 || iy >= H) continue;               // wave-uniform
        const float* row = src + (size_t)iy * W;
        f32x2 v[4];
        float left[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int ox = ox0 + 64 * q;
          const bool in = 2 * ox + 1 < W;              // W even: both columns exist or neither
          v[q] = in ? *reinterpret_cast<const f32x2*>(row + 2 * ox) : f32x2{-INFINITY, -INFINITY};
          left[q] = (lane == 0 && ox > 0 && 2 * ox - 1 < W) ? row[2 * ox - 1] : -INFINITY;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float nb = __shfl_up(v[q][1], 1, 64);
          const float l = lane == 0 ? left[q] : nb;
          m[q] = pool_max(pool_max(pool_max(m[q], l), v[q][0]), v[q][1]);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (ox0 + 64 * q < OW) dst[ox0 + 64 * q] = m[q];
    }
    return;
  }
  // generic widths: four 64-column chunks per pass, 36 independent loads in flight per lane
  for (int ox0 = lane; ox0 < OW; ox0 += 256) {
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int iy = oy * 2 - 1 + dy;
      const bool rok = iy >= 0 && iy < H;
      const float* row = src + (size_t)(rok ? iy : 0) * W;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const int ix = (ox0 + 64 * q) * 2 - 1 + dx;
          const bool ok = rok && ix >= 0 && ix < W;
          const float v = ok ? row[ix] : -INFINITY;
          m[q] = pool_max(m[q], v);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (ox0 + 64 * q < OW) dst[ox0 + 64 * q] = m[q];
  }
}

// AdaptiveAvgPool2d(1) + flatten + fc, modeling/resnet.py:288-290; one 16-wave workgroup per image, four channel
// planes in flight per wave (the means are plain sequential-lane sums: deterministic)
__global__ void __launch_bounds__(1024) avgpool_fc_kernel(const float* __restrict__ x, const float* __restrict__ fw,
                                                           const float* __restrict__ fb, float* __restrict__ out,
                                                           int C, int HW, int out_dim, uint32_t* status) {
  __shared__ float pooled[512];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* src = x + (size_t)n * C * HW;
  const float inv = 1.0f / (float)HW;
  for (int c0 = wave * 4; c0 < C; c0 += 64) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = lane; i < HW; i += 64) {
#pragma unroll
      for (int q = 0; q < 4; ++q) s[q] += (c0 + q < C) ? src[(size_t)(c0 + q) * HW + i] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float t = wave_sum(s[q]);
      if (lane == 0 && c0 + q < C) pooled[c0 + q] = t * inv;
    }
  }
  __syncthreads();
  bool bad = false;
  for (int j = wave; j < out_dim; j += 16) {
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += fw[(size_t)j * C + c] * pooled[c];
    s = wave_sum(s);
    if (lane == 0) {
      const float o = s + fb[j];
      out[(size_t)n * out_dim + j] = o;
      bad |= out_of_fp16(o);
    }
  }
  range_flag(status, bad);
}

int maxpool_launch(const float* x, float* y, int planes, int H, int W, int OH, int OW, hipStream_t s) {
  maxpool_kernel<<<dim3(planes, ceil_div(OH, 4)), dim3(256), 0, s>>>(x, y, planes, H, W, OH, OW);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

// the same on a map in the cell layout (conv2d_hs.hip: per image [C / 8][hi, lo][HW] cells of eight fp16 channels): one cell
// group per wave at a time, value = hi + lo / 2^11, the same lane-strided partial sums and wave reduction per channel
__global__ void __launch_bounds__(1024) avgpool_fc_cells_kernel(const uint4* __restrict__ x, const float* __restrict__ fw,
                                                                 const float* __restrict__ fb, float* __restrict__ out,
                                                                 int C, int HW, int out_dim, uint32_t* status) {
  typedef _Float16 h8 __attribute__((ext_vector_type(8)));
  __shared__ float pooled[512];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint4* src = x + (size_t)n * (C / 8) * 2 * HW;
  const float inv = 1.0f / (float)HW;
  for (int g = wave; g < C / 8; g += 16) {
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = lane; i < HW; i += 64) {
      const h8 hi = __builtin_bit_cast(h8, src[(size_t)(2 * g) * HW + i]);
      const h8 lo = __builtin_bit_cast(h8, src[(size_t)(2 * g + 1) * HW + i]);
#pragma unroll
      for (int q = 0; q < 8; ++q) s[q] += (float)hi[q] + (float)lo[q] * (1.f / 2048.f);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float t = wave_sum(s[q]);
      if (lane == 0) pooled[8 * g + q] = t * inv;
    }
  }
  __syncthreads();
  bool bad = false;
  for (int j = wave; j < out_dim; j += 16) {
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += fw[(size_t)j * C + c] * pooled[c];
    s = wave_sum(s);
    if (lane == 0) {
      const float o = s + fb[j];
      out[(size_t)n * out_dim + j] = o;
      bad |= out_of_fp16(o);
    }
  }
  range_flag(status, bad);
}

int avgpool_fc_launch(const float* x, const float* fw, const float* fb, float* out, int batch, int C, int HW, int out_dim,
                      hipStream_t s, int x_cells, uint32_t* status) {
  ADX_REQUIRE(C <= 512, "avgpool_fc: at most 512 channels");
  if (x_cells) {
    ADX_REQUIRE(C % 8 == 0, "avgpool_fc: the cell layout holds channels in groups of eight");
    avgpool_fc_cells_kernel<<<dim3(batch), dim3(1024), 0, s>>>(reinterpret_cast<const uint4*>(x), fw, fb, out, C, HW, out_dim, status);
    ADX_LAUNCH_CHECK();
    return ADX_OK;
  }
  avgpool_fc_kernel<<<dim3(batch), dim3(1024), 0, s>>>(x, fw, fb, out, C, HW, out_dim, status);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

}  // namespace adx

namespace adx {

static int conv2d_launch(const ConvSpec& L, const float* base, const float* x, const float* res, float* y, int N, int H,
                         int W, int relu, hipStream_t s, int fmt = 0) {
  return conv2d_launch_raw(L, x, base + L.o_w, base + L.o_scale, base + L.o_shift, res, y, N, H, W, relu, s, nullptr, 0, nullptr, 0,
                           nullptr, fmt);
}

static thread_local float* t_split_scratch = nullptr;
static thread_local size_t t_split_floats = 0;
void conv2d_set_split_scratch(float* p, size_t floats) { t_split_scratch = p; t_split_floats = p != nullptr ? floats : 0; }
// compute units of the calling thread's current device, asked once per device (devices folded modulo 64, like DeviceOnce)
int device_cus(int* cus) {
  static std::atomic<int> known[64];
  int dev = 0;
  ADX_CHECK_HIP(hipGetDevice(&dev));
  std::atomic<int>& n = known[dev & 63];
  if (n.load(std::memory_order_relaxed) == 0) {
    hipDeviceProp_t prop;
    ADX_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
    n.store(prop.multiProcessorCount > 8 ? prop.multiProcessorCount : 8, std::memory_order_relaxed);
  }
  *cus = n.load(std::memory_order_relaxed);
  return ADX_OK;
}
static thread_local int t_reserve_cus = -1;
void conv2d_set_reserve_cus(int reserve) { t_reserve_cus = reserve; }
int launch_cus(int* cus) {
  int dev = 0;
  const int rc = device_cus(&dev);
  if (rc != ADX_OK) return rc;
  const DebugSwitches& sw = debug_switches();
  *cus = hs_usable_cus(dev, t_reserve_cus >= 0 ? t_reserve_cus : sw.hs_reserve_cus, sw.hs_grid_cap);
  return ADX_OK;
}
static thread_local uint32_t* t_status = nullptr;
void conv2d_set_status(uint32_t* word) { t_status = word; }
uint32_t* conv2d_status() { return t_status; }

int conv2d_launch_raw(const ConvSpec& L, const float* x, const float* w, const float* scale, const float* shift,
                      const float* res, float* y, int N, int H, int W, int relu, hipStream_t s, const uint32_t* x_amax,
                      int x_amax_n, float* stats_part, size_t stats_floats, int* stats_p, int fmt, const BnBwdStats* bst) {
  if (stats_p != nullptr) *stats_p = 0;
  Conv2dArgs a;
  a.x = x; a.w = w; a.scale = scale; a.shift = shift; a.res = res; a.y = y; a.x_amax = x_amax; a.x_amax_n = x_amax_n;
  a.w_ds = nullptr; a.scale_ds = nullptr; a.shift_ds = nullptr; a.y_ds = nullptr;
  a.N = N; a.Cin = L.cin; a.H = H; a.W = W; a.Cout = L.cout;
  a.OH = conv_out_dim(H, L.k, L.stride, L.pad); a.OW = conv_out_dim(W, L.k, L.stride, L.pad);
  a.KH = L.k; a.KW = L.k; a.stride = L.stride; a.pad = L.pad; a.relu = relu;
  a.cin_pad = L.cin_pad; a.cc = L.cc;
  a.x_u8 = nullptr;
  a.d2s_cin = 0; a.d2s_h = 0; a.d2s_w = 0; a.stem_seg_tiles = 0; a.stem_nseg = 1;
  a.status = t_status;
  a.ksplit = 1; a.cper = 0; a.part = t_split_scratch; a.part_stride = 0;
  a.stats_part = nullptr; a.stats_p = 0;
  a.bs_raw = a.bs_out = a.bs_mean = a.bs_rstd = a.bs_gamma = a.bs_beta = nullptr; a.bs_mask = 0; a.bs_bits = nullptr; a.res_bits = nullptr;
  if (bst != nullptr) {
    ADX_REQUIRE(bst->raw && bst->mean && bst->rstd && bst->gamma && bst->beta && (bst->mask == 2 || (bst->mask == 1 && (bst->out || bst->bits))),
                "conv2d: incomplete BatchNorm-backward statistics request");
    ADX_REQUIRE(scale == nullptr && relu == 0, "conv2d: BatchNorm-backward statistics belong to data-gradient launches");
    a.bs_raw = bst->raw; a.bs_out = bst->out; a.bs_mean = bst->mean; a.bs_rstd = bst->rstd; a.bs_gamma = bst->gamma;
    a.bs_beta = bst->beta; a.bs_mask = bst->mask; a.bs_bits = bst->mask == 1 ? bst->bits : nullptr;
    a.res_bits = bst->res_bits;
  }
  a.x_cells = (fmt & kFmtXCells) != 0; a.y_cells = (fmt & kFmtYCells) != 0; a.res_cells = (fmt & kFmtResCells) != 0 && res != nullptr;
  // everything the 3x3 stride-1 split-fp16 kernels decide about this launch (family none: another kernel's)
  Hs3x3Query q;
  q.N = N; q.H = H; q.W = W; q.fmt = fmt;
  q.stats_floats = stats_part != nullptr && stats_p != nullptr ? stats_floats : 0;
  q.bst_mask = a.bs_mask; q.bst_bits = a.bs_bits != nullptr;
  q.x_scale = x_amax == nullptr ? kXScaleNone : (x_amax_n < 0 ? kXScalePre : kXScaleDynamic);
  q.affine = scale != nullptr; q.relu = relu != 0; q.has_res = res != nullptr;
  q.y_aligned = (reinterpret_cast<uintptr_t>(y) & 15) == 0; q.res_aligned = (reinterpret_cast<uintptr_t>(res) & 15) == 0;
  q.split_floats = t_split_floats;
  if (L.k == 3 && L.stride == 1) {      // (the persistent grid of the 16x16x32 kernel)
    const int rc = launch_cus(&q.cus);
    if (rc != ADX_OK) return rc;
  }
  const Hs3x3Plan plan = conv2d_hs3x3_plan(L, q);
  ADX_REQUIRE(a.res_bits == nullptr || (res != nullptr && L.dgrad && plan.stats == 2),
              "conv2d: a masked residual belongs to a data-gradient launch with the statistics epilogue");
  ADX_REQUIRE(plan.admitted, "conv2d: the cell layout belongs to plain launches of the pipelined 3x3 kernel (%d -> %d, k%d s%d)", L.cin, L.cout,
              L.k, L.stride);
  if (conv2d_hs_eligible(L)) {
    if (plan.stats != 0) {
      a.stats_part = stats_part;
      a.stats_p = plan.stats_tiles;
      *stats_p = plan.stats_tiles;
    }
    return conv2d_hs_launch(L, a, s, &plan);
  }
  const int rows = (L.stride == 1 && L.k == 3) ? 2 : 1;   // 8-row tiles for the 3x3 stride-1 convs
  const int th = 4 * rows;
  a.tiles_x = ceil_div(a.OW, kTileW); a.tiles_y = ceil_div(a.OH, th); a.cout_tiles = L.cout / kCoutT;
  a.PH = (th - 1) * L.stride + L.k; a.PW = (kTileW - 1) * L.stride + L.k;
  a.PWp = a.PW;
  ADX_REQUIRE(L.cin % L.cc == 0 || L.cin < L.cc, "conv2d: cin %d must be < %d or a multiple of it", L.cin, L.cc);
  ADX_REQUIRE((size_t)L.cin * H * W < (1u << 31), "conv2d: image plane too large for 32-bit gather offsets");
  const size_t np = (size_t)a.cc * a.PH * a.PW;
  const size_t lds = sizeof(float) * ((np + 255) / 256 * 256 + (size_t)L.k * L.k * a.cc * kCoutT + 2 * kCoutT);
  ADX_REQUIRE(lds <= kMaxLds, "conv2d: LDS %zu bytes too large", lds);
  const size_t grid = (size_t)a.cout_tiles * a.tiles_x * a.tiles_y * N;
  ADX_REQUIRE(grid < (1u << 31), "conv2d: grid too large");
  static std::atomic<uint64_t> attr_set{0};  // dynamic LDS above 64 KB must be opted into once per kernel
  if (DeviceOnce once{attr_set}; once) {
    const void* fns[5] = {reinterpret_cast<const void*>(&conv2d_kernel<1, 3, 2>), reinterpret_cast<const void*>(&conv2d_kernel<2, 3, 1>),
                          reinterpret_cast<const void*>(&conv2d_kernel<2, 1, 1>), reinterpret_cast<const void*>(&conv2d_kernel<2, 7, 1>),
                          reinterpret_cast<const void*>(&conv2d_kernel<1, 1, 1>)};
    for (const void* f : fns) ADX_CHECK_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds));
    once.commit();
  }
  const dim3 g((unsigned)grid), blk(256);
  if (L.stride == 1 && L.k == 3) conv2d_kernel<1, 3, 2><<<g, blk, lds, s>>>(a);
  else if (L.stride == 2 && L.k == 3) conv2d_kernel<2, 3, 1><<<g, blk, lds, s>>>(a);
  else if (L.stride == 2 && L.k == 1) conv2d_kernel<2, 1, 1><<<g, blk, lds, s>>>(a);
  else if (L.stride == 2 && L.k == 7) conv2d_kernel<2, 7, 1><<<g, blk, lds, s>>>(a);
  else if (L.stride == 1 && L.k == 1) conv2d_kernel<1, 1, 1><<<g, blk, lds, s>>>(a);
  else {
    set_error("conv2d: no kernel for k=%d stride=%d (ResNet-34 uses 3x3 s1, 3x3 s2, 1x1 s2, 7x7 s2)", L.k, L.stride);
    return ADX_ERR_INVALID;
  }
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

}  // namespace adx

using namespace adx;

static int spec_from_desc(const adx_conv2d_desc* d, ConvSpec* L) {
  ADX_REQUIRE(d != nullptr, "conv2d: null descriptor");
  ADX_REQUIRE(d->cin >= 1 && d->cout >= 64 && d->cout % kCoutT == 0, "conv2d: cout %d must be a multiple of %d", d->cout,
              kCoutT);
  ADX_REQUIRE(d->k >= 1 && d->k <= 7 && (d->stride == 1 || d->stride == 2) && d->pad >= 0 && d->pad <= 3,
              "conv2d: unsupported k/stride/pad %d/%d/%d", d->k, d->stride, d->pad);
  memset(L, 0, sizeof(*L));
  L->cin = d->cin; L->cout = d->cout; L->k = d->k; L->stride = d->stride; L->pad = d->pad;
  L->cc = d->cin >= 16 ? 16 : 4;
  L->cin_pad = round_up(d->cin, L->cc);
  return ADX_OK;
}

extern "C" {

size_t adx_conv2d_packed_bytes(const adx_conv2d_desc* d) {
  ConvSpec L;
  if (spec_from_desc(d, &L) != ADX_OK) return 0;
  return sizeof(float) * (conv2d_hs_eligible(L) ? conv2d_packed_floats(L) : (size_t)L.k * L.k * L.cin_pad * L.cout);
}

int adx_conv2d_pack(const adx_conv2d_desc* d, const float* w, float* packed, adx_stream stream) {
  ConvSpec L;
  int rc = spec_from_desc(d, &L);
  if (rc != ADX_OK) return rc;
  ADX_REQUIRE(w && packed, "adx_conv2d_pack: null pointer");
  return conv2d_pack_spec(L, w, packed, 0, (hipStream_t)stream);
}

int adx_conv2d_forward(const adx_conv2d_desc* d, const float* x, const float* packed_w, const float* scale,
                       const float* shift, const float* res, float* y, int32_t n, int32_t h, int32_t w, int32_t relu,
                       adx_stream stream) {
  ConvSpec L;
  int rc = spec_from_desc(d, &L);
  if (rc != ADX_OK) return rc;
  ADX_REQUIRE(x && packed_w && y, "adx_conv2d_forward: null tensor");
  ADX_REQUIRE((scale == nullptr) == (shift == nullptr), "adx_conv2d_forward: scale and shift go together");
  ADX_REQUIRE(n >= 1 && h + 2 * d->pad >= d->k && w + 2 * d->pad >= d->k, "adx_conv2d_forward: input too small");
  return conv2d_launch_raw(L, x, packed_w, scale, shift, res, y, n, h, w, relu, (hipStream_t)stream);
}

int adx_conv2d_cells_supported(const adx_conv2d_desc* d, int32_t n, int32_t h, int32_t w) {
  ConvSpec L;
  if (d == nullptr || spec_from_desc(d, &L) != ADX_OK) return 0;
  return conv2d_hs3x3_plain(L, n, h, w) ? 1 : 0;
}

int adx_conv2d_forward_cells(const adx_conv2d_desc* d, const void* x, const float* packed_w, const float* scale,
                             const float* shift, const void* res, void* y, int32_t n, int32_t h, int32_t w, int32_t relu,
                             int32_t fmt, adx_stream stream) {
  ConvSpec L;
  int rc = spec_from_desc(d, &L);
  if (rc != ADX_OK) return rc;
  ADX_REQUIRE(x && packed_w && y, "adx_conv2d_forward_cells: null tensor");
  ADX_REQUIRE((scale == nullptr) == (shift == nullptr), "adx_conv2d_forward_cells: scale and shift go together");
  ADX_REQUIRE(fmt >= 0 && fmt <= 7 && (fmt & kFmtYCells), "adx_conv2d_forward_cells: fmt %d (the output is a cell tensor)", fmt);
  ADX_REQUIRE(conv2d_hs3x3_plain(L, n, h, w), "adx_conv2d_forward_cells: not a plain launch of the pipelined 3x3 kernel "
              "(adx_conv2d_cells_supported)");
  return conv2d_launch_raw(L, (const float*)x, packed_w, scale, shift, (const float*)res, (float*)y, n, h, w, relu,
                           (hipStream_t)stream, nullptr, 0, nullptr, 0, nullptr, fmt);
}

static int block_s2_specs(int32_t cin, int32_t cout, ConvSpec* c1, ConvSpec* ds, const char* who) {
  const adx_conv2d_desc d1{cin, cout, 3, 2, 1}, dd{cin, cout, 1, 2, 0};
  int rc = spec_from_desc(&d1, c1);
  if (rc == ADX_OK) rc = spec_from_desc(&dd, ds);
  if (rc != ADX_OK) return rc;
  ADX_REQUIRE(resnet_fuses_ds(*c1, *ds), "%s: %d -> %d is no block entry the split-fp16 kernels fuse (cin %% 16, cout %% 64, not ADX_CONV_EXACT=1)",
              who, cin, cout);
  return ADX_OK;
}

int adx_conv2d_pack_ds(int32_t cin, int32_t cout, const float* w, float* packed, adx_stream stream) {
  ConvSpec c1, ds;
  const int rc = block_s2_specs(cin, cout, &c1, &ds, "adx_conv2d_pack_ds");
  if (rc != ADX_OK) return rc;
  ADX_REQUIRE(w && packed, "adx_conv2d_pack_ds: null pointer");
  return conv2d_hs_pack(ds, w, packed, 0, (hipStream_t)stream);
}

int adx_conv2d_block_s2_cells(int32_t cin, int32_t cout, const void* x, const float* packed_w1, const float* scale1, const float* shift1,
                              void* y1, const float* packed_wd, const float* scaled, const float* shiftd, void* yd, int32_t n, int32_t h,
                              int32_t w, int32_t flags, adx_stream stream) {
  ConvSpec c1, ds;
  const int rc = block_s2_specs(cin, cout, &c1, &ds, "adx_conv2d_block_s2_cells");
  if (rc != ADX_OK) return rc;
  ADX_REQUIRE(x && packed_w1 && y1 && packed_wd && yd, "adx_conv2d_block_s2_cells: null tensor");
  ADX_REQUIRE((scale1 == nullptr) == (shift1 == nullptr) && (scaled == nullptr) == (shiftd == nullptr),
              "adx_conv2d_block_s2_cells: scale and shift go together");
  ADX_REQUIRE(n >= 1 && h >= 1 && w >= 1 && flags >= 0 && flags <= 1, "adx_conv2d_block_s2_cells: bad shape %d x %d x %d or flags %d", n, h, w, flags);
  ADX_REQUIRE((size_t)n * cin * h * w * sizeof(float) < 0xC0000000u, "adx_conv2d_block_s2_cells: the input exceeds the 32-bit byte offsets");
  return conv2d_hs_launch_block_s2(c1, ds, (const float*)x, packed_w1, scale1, shift1, (float*)y1, packed_wd, scaled, shiftd, (float*)yd, n, h, w,
                                   (hipStream_t)stream, 1, 1, 1, (flags & 1) != 0);
}

int adx_conv2d_stem_pool(const void* x, int32_t x_u8, const float* packed_w, const float* scale, const float* shift,
                         const float* mean, const float* stdv, void* y, int32_t n, int32_t h, int32_t w, int32_t y_cells,
                         adx_stream stream) {
  ConvSpec L{};
  L.cin = 3; L.cout = 64; L.k = 7; L.stride = 2; L.pad = 3; L.cc = 4; L.cin_pad = 4;
  ADX_REQUIRE(x && packed_w && scale && shift && y, "adx_conv2d_stem_pool: null tensor");
  ADX_REQUIRE(n >= 1 && h >= 1 && w >= 1, "adx_conv2d_stem_pool: bad shape %d x %d x %d", n, h, w);
  ADX_REQUIRE(conv2d_hs_eligible(L), "adx_conv2d_stem_pool: the fused stem + pool is a split-fp16 kernel (unavailable with ADX_CONV_EXACT=1)");
  ADX_REQUIRE(!x_u8 || (mean && stdv), "adx_conv2d_stem_pool: uint8 frames need mean / std");
  return conv2d_hs_stem_pool(L, x_u8 ? nullptr : (const float*)x, packed_w, scale, shift, (float*)y, n, h, w, (hipStream_t)stream,
                             x_u8 ? (const uint8_t*)x : nullptr, mean, stdv, y_cells ? 1 : 0);
}

int adx_resnet_create(int32_t out_dim, adx_resnet** out) {
  ADX_REQUIRE(out != nullptr && out_dim >= 1 && out_dim <= 4096, "adx_resnet_create: bad argument");
  adx_resnet* r = new adx_resnet();
  r->out_dim = out_dim;
  int t = 0;
  size_t off = 0;
  auto add = [&](int cin, int cout, int k, int stride, int pad) {
    ConvSpec L{};
    L.cin = cin; L.cout = cout; L.k = k; L.stride = stride; L.pad = pad;
    L.t_w = t++; L.t_g = t++; L.t_b = t++; L.t_m = t++; L.t_v = t++;
    L.cc = cin >= 16 ? 16 : 4;
    L.cin_pad = round_up(cin, L.cc);
    L.fuse_with = -1;
    L.o_w = off; off = al64(off + (conv2d_hs_eligible(L) ? conv2d_packed_floats(L) : (size_t)k * k * L.cin_pad * cout));
    L.o_scale = off; off = al64(off + cout);
    L.o_shift = off; off = al64(off + cout);
    r->convs.push_back(L);
  };
  add(3, 64, 7, 2, 3);
  const int planes[4] = {64, 128, 256, 512}, nblk[4] = {3, 4, 6, 3};
  int inpl = 64;
  for (int li = 0; li < 4; ++li)
    for (int bi = 0; bi < nblk[li]; ++bi) {
      const int stride = (li > 0 && bi == 0) ? 2 : 1;
      add(inpl, planes[li], 3, stride, 1);
      add(planes[li], planes[li], 3, 1, 1);
      const int ds = (stride != 1 || inpl != planes[li]) ? 1 : 0;
      if (ds) {
        add(inpl, planes[li], 1, stride, 0);
        r->convs.back().fuse_with = (int)r->convs.size() - 3;   // its block's conv1
      }
      r->block_has_ds.push_back(ds);
      inpl = planes[li];
    }
  r->t_fcw = t++; r->t_fcb = t++;
  r->n_tensors = t;
  r->o_fcw = off; off = al64(off + (size_t)out_dim * 512);
  r->o_fcb = off; off = al64(off + out_dim);
  r->packed_floats = off;
  *out = r;
  return ADX_OK;
}

void adx_resnet_destroy(adx_resnet* r) {
  if (r == nullptr) return;
  for (auto& st : r->side) if (st != nullptr) (void)hipStreamDestroy(st);
  if (r->ev_fork != nullptr) (void)hipEventDestroy(r->ev_fork);
  for (auto& ev : r->ev_join) if (ev != nullptr) (void)hipEventDestroy(ev);
  delete r;
}
int adx_resnet_num_tensors(const adx_resnet* r) { return r ? r->n_tensors : 0; }

int32_t adx_resnet_status_words(const adx_resnet* r) {
  ADX_REQUIRE(r != nullptr, "adx_resnet_status_words: null handle");
  return (int32_t)r->block_has_ds.size() + 3;
}

int adx_resnet_set_status(adx_resnet* r, uint32_t* words) {
  ADX_REQUIRE(r != nullptr, "adx_resnet_set_status: null handle");
  r->status = words;
  return ADX_OK;
}

const char* adx_resnet_status_name(const adx_resnet* r, int32_t g) {
  static const char* const kBlocks[16] = {"block0", "block1", "block2",  "block3",  "block4",  "block5",  "block6",  "block7",
                                          "block8", "block9", "block10", "block11", "block12", "block13", "block14", "block15"};
  if (r == nullptr) { set_error("adx_resnet_status_name: null handle"); return nullptr; }
  const int nb = (int)r->block_has_ds.size();
  if (g < 0 || g >= nb + 3) { set_error("adx_resnet_status_name: group %d outside [0, %d)", g, nb + 3); return nullptr; }
  return g == 0 ? "stem" : g <= nb ? kBlocks[g - 1] : g == nb + 1 ? "fc" : "weights";
}

// the executor's launches between construction and destruction write the given status word (conv2d_set_status)
struct StatusScope {
  explicit StatusScope(uint32_t* w) { conv2d_set_status(w); }
  void set(uint32_t* w) { conv2d_set_status(w); }
  ~StatusScope() { conv2d_set_status(nullptr); }
};
size_t adx_resnet_packed_bytes(const adx_resnet* r) { return r ? r->packed_floats * sizeof(float) : 0; }

int adx_resnet_pack(adx_resnet* r, const float* const* T, int32_t n, void* packed, adx_stream stream) {
  ADX_REQUIRE(r && T && packed, "adx_resnet_pack: null argument");
  ADX_REQUIRE(n == r->n_tensors, "adx_resnet_pack: expected %d tensors, got %d", r->n_tensors, n);
  for (int i = 0; i < n; ++i) ADX_REQUIRE(T[i] != nullptr, "adx_resnet_pack: tensor %d is null", i);
  hipStream_t s = (hipStream_t)stream;
  float* base = (float*)packed;
  StatusScope status_scope(r->status != nullptr ? r->status + r->block_has_ds.size() + 2 : nullptr);   // "weights"
  for (const ConvSpec& L : r->convs) {
    // a downsample conv that rides on its block's split-fp16 conv1 is packed in that kernel's layout
    const bool fused = L.fuse_with >= 0 && resnet_fuses_ds(r->convs[L.fuse_with], L);
    int rc = fused ? conv2d_hs_pack(L, T[L.t_w], base + L.o_w, 0, s) : conv2d_pack_spec(L, T[L.t_w], base + L.o_w, 0, s);
    if (rc != ADX_OK) return rc;
    bn_fold_kernel<<<dim3(ceil_div(L.cout, 256)), dim3(256), 0, s>>>(T[L.t_g], T[L.t_b], T[L.t_m], T[L.t_v],
                                                                     base + L.o_scale, base + L.o_shift, L.cout);
    ADX_LAUNCH_CHECK();
  }
  ADX_CHECK_HIP(hipMemcpyAsync(base + r->o_fcw, T[r->t_fcw], (size_t)r->out_dim * 512 * sizeof(float),
                               hipMemcpyDeviceToDevice, s));
  ADX_CHECK_HIP(hipMemcpyAsync(base + r->o_fcb, T[r->t_fcb], (size_t)r->out_dim * sizeof(float),
                               hipMemcpyDeviceToDevice, s));
  r->packed_once = true;
  return ADX_OK;
}

// workspace: the stem output, then three rotating buffers sized for the post-maxpool map
extern "C++" ResnetLayout adx::resnet_layout(int batch, int h, int w) {
  ResnetLayout l;
  l.h1 = conv_out_dim(h, 7, 2, 3); l.w1 = conv_out_dim(w, 7, 2, 3);
  l.h2 = conv_out_dim(l.h1, 3, 2, 1); l.w2 = conv_out_dim(l.w1, 3, 2, 1);
  l.stem = al64((size_t)batch * 64 * l.h1 * l.w1);
  l.act = al64((size_t)batch * 64 * l.h2 * l.w2);
  return l;
}

size_t adx_resnet_workspace_bytes(const adx_resnet* r, int32_t batch, int32_t h, int32_t w) {
  if (!r || batch < 1 || h < 32 || w < 32) return 0;
  return resnet_layout(batch, h, w).floats() * sizeof(float);
}

// The plan of one eval forward (conv2d_internal.h states the format rule).
// Sub-batches on streams of their own (round 5).  A launch of the pipelined 3x3 kernels is one workgroup per CU and tile, and at
// B = 64 the tile counts are 1.8 (256 channels) / 3.6 (128) / 0.94 (512) times the 256 CUs: the last round of every launch leaves
// 6-10 % of the chip idle and the next launch cannot start before it ends.  Two half batches are two independent chains of
// launches: while one's last workgroups run, the other's fill the idle CUs (a second workgroup of these kernels does not fit
// a CU, so the co-scheduled kernel gets exactly the idle ones).  Same kernels, same per-image arithmetic: the features are bit
// for bit those of the single-stream pass wherever the tile modes agree.  Weights are read once per sub-batch instead of once.
// (Running stem, layer1 and layer2's first block in batch chunks of 16, so that a 59 MB activation is still in the 256 MB
// Infinity Cache when the next launch reads it, was measured: layer1's convs already find most of their input there at
// B = 64 -- inside a pass they take 0.20 ms where the same launch repeated on fixed buffers takes 0.25 -- and the chunked
// stem launch has too few workgroups: +-1 % end to end for 2..4 chunks, -13 % for 8.  Not kept.)
extern "C++" int adx::resnet_eval_plan(const adx_resnet& r, const ResnetEvalQuery& q, ResnetEvalPlan* plan, const DebugSwitches& sw) {
  const int nblocks = (int)r.block_has_ds.size();
  ADX_REQUIRE(q.batch >= 1 && q.h >= 32 && q.w >= 32, "adx_resnet_forward: image %dx%d (batch %d) too small", q.h, q.w, q.batch);
  ADX_REQUIRE(!r.convs.empty() && nblocks <= kResnetMaxBlocks, "adx_resnet_forward: %d BasicBlocks, the plan holds %d", nblocks, kResnetMaxBlocks);
  // the stem + max-pool run as one launch wherever the split-fp16 stem kernel exists; the unpooled stem map is never written then
  // and its region is the split-reduction scratch of the convs, one slice per sub-batch
  const bool stem_fused = conv2d_hs_eligible(r.convs[0], sw);
  ADX_REQUIRE(stem_fused || !q.u8,
              "adx_resnet_forward_u8: the uint8 front-end lives in the split-fp16 stem kernel (unavailable with ADX_CONV_EXACT=1)");
  ResnetEvalPlan& p = *plan;
  p = ResnetEvalPlan{};
  p.lay = resnet_layout(q.batch, q.h, q.w);
  // not inside a stream capture: a replayed graph with the forked branches measured 2 % SLOWER per tick than the single chain
  // (profiles/README.md, round 5), and streams are not created while capturing
  // The sub-batches and the reserve are ONE choice: what runs beside the pass (the caller's other streams: the temporal stack of the
  // next tick) gets CUs either between the launches of two interleaved chains or on CUs the persistent launches never take.
  // Candidates at B = 64: {two sub-batch streams, one chain} x {reserve 0, 16} (profiles/README.md, "The unit walk").
  p.reserve_cus = kEvalReserveCus[0];
  if (q.batch >= 32 && !sw.check_range && stem_fused && !q.capturing) {
    p.nsub = std::min(sw.resnet_streams, adx_resnet::kMaxSub);
    while (p.nsub > 1 && q.batch / p.nsub < 16) --p.nsub;
    p.reserve_cus = kEvalReserveCus[1];
  }
  if (sw.hs_reserve_cus >= 0) p.reserve_cus = sw.hs_reserve_cus;        // ADX_HS_RESERVE_CUS pins it for every pass
  // The stem and the first layer (the blocks in front of the first downsample block) run as ONE chain on the whole batch, the fork
  // comes behind them: their launches are thousands of two-per-CU workgroups whose last round hardly matters, and split they
  // only stream their operands twice (-1.6 % per faithful step, profiles/README.md).  Only blocks of the FIRST layer: their maps
  // have the pooled map's per-image size, so the whole-batch tensors they leave are laid out exactly like the sub-batches'
  // regions.  ADX_RESNET_SPLIT_FROM=<block> can only shorten the prefix.
  if (p.nsub > 1) {
    while (p.first_split < nblocks && !r.block_has_ds[p.first_split]) ++p.first_split;
    if (sw.resnet_split_from >= 0) p.first_split = std::min(sw.resnet_split_from, p.first_split);
  }
  int c1_of[kResnetMaxBlocks + 1];          // index of block b's conv1 in r.convs (conv2 and the downsample follow it)
  c1_of[0] = 1;
  for (int b = 0; b < nblocks; ++b) c1_of[b + 1] = c1_of[b] + 2 + (r.block_has_ds[b] ? 1 : 0);

  auto plain = [&](const ConvSpec& c, int nf, int H, int W) {
    Hs3x3Query hq;
    hq.N = nf; hq.H = H; hq.W = W; hq.fmt = kFmtXCells | kFmtYCells;
    return conv2d_hs3x3_plan(c, hq, sw).admitted;
  };
  auto fuses = [&](int b) { return r.block_has_ds[b] && resnet_fuses_ds(r.convs[c1_of[b]], r.convs[c1_of[b] + 2], sw); };
  auto reads_cells = [&](int b, int nf, int H, int W) {       // block b on an input map of H x W
    const ConvSpec& c1 = r.convs[c1_of[b]];
    if (r.block_has_ds[b]) return fuses(b);
    return c1.stride == 1 && plain(c1, nf, H, W) && plain(r.convs[c1_of[b] + 1], nf, H, W);
  };
  struct Edge { int buf, H, W; bool cells; };
  // the stem (g.stem) and blocks [b0, b1) of one segment, from the edge `at` on; leaves the edge it ends with
  auto chain = [&](ResnetSegment& g, int b0, int b1, Edge& at) -> int {
    if (g.stem) at = Edge{0, p.lay.h2, p.lay.w2, false};
    bool reads = b0 < nblocks && reads_cells(b0, g.nf, at.H, at.W);     // of the block at hand, asked once: as its producer's reader
    if (g.stem) {
      g.stem_fused = stem_fused;
      at.cells = g.pooled_cells = stem_fused && reads;
    }
    for (int b = b0; b < b1; ++b) {
      ResnetBlockStep& t = g.steps[g.nsteps++];
      const ConvSpec& c1 = r.convs[c1_of[b]];
      const ConvSpec& c2 = r.convs[c1_of[b] + 1];
      const bool has_ds = r.block_has_ds[b] != 0;
      t.block = b; t.c1 = c1_of[b]; t.status = 1 + b;
      t.H = at.H; t.W = at.W;
      t.OH = conv_out_dim(t.H, 3, c1.stride, 1); t.OW = conv_out_dim(t.W, 3, c1.stride, 1);
      t.fused_ds = fuses(b);
      // With a downsample the identity lives in the third buffer and the result overwrites the block's input (dead by then)
      t.in = at.buf; t.mid = (at.buf + 1) % 3;
      t.id = has_ds ? (at.buf + 2) % 3 : at.buf;
      t.out = has_ds ? at.buf : (at.buf + 2) % 3;
      const bool c2_plain = plain(c2, g.nf, t.OH, t.OW), next_reads = b + 1 < nblocks && reads_cells(b + 1, g.nf, t.OH, t.OW);
      t.in_cells = at.cells;              // the producer's decision
      t.mid_cells = t.fused_ds ? c2_plain : (!has_ds && reads);
      t.id_cells = has_ds ? (t.fused_ds && t.mid_cells) : t.in_cells;
      t.out_cells = c2_plain && (b + 1 == nblocks || next_reads);
      // every cell operand has a reader of cells: the block itself (its input), and whoever reads conv2's output when conv2 reads any
      ADX_REQUIRE((!t.in_cells || reads) && (t.out_cells || !(t.mid_cells || t.id_cells)),
                  "adx_resnet_forward: internal error (cell-layout input of a launch that cannot read it): BasicBlock %d at batch %d of %d", b,
                  g.nf, q.batch);
      at = Edge{t.out, t.OH, t.OW, t.out_cells};
      reads = next_reads;
    }
    g.final_buf = at.buf; g.final_h = at.H; g.final_w = at.W; g.final_cells = at.cells;
    return ADX_OK;
  };

  const size_t scratch_per = stem_fused ? ((size_t)q.batch * 64 * p.lay.h1 * p.lay.w1 / p.nsub) & ~(size_t)63 : 0;
  Edge whole{};
  if (p.first_split > 0) {
    ResnetSegment& g = p.seg[p.nseg++];
    g.id = 0; g.n0 = 0; g.n = g.nf = q.batch; g.stream = 0;
    g.scratch_off = 0; g.scratch_floats = scratch_per;       // (sub-batch 0's slice: it starts behind the prefix on the same stream)
    g.stem = true;
    const int rc = chain(g, 0, p.first_split, whole);
    if (rc != ADX_OK) return rc;
  }
  // a sub-batch owns the SAME region of every rotating buffer at every layer (its first image's slot of the largest map, the
  // pooled one; the images of a layer are packed from there): sub-batches run on streams of their own and are at different
  // layers at the same time, so a region that moved with the layer's per-image size would overlap another sub-batch's
  for (int k = 0, n0 = 0; k < p.nsub; ++k) {
    ResnetSegment& g = p.seg[p.nseg++];
    g.id = 1 + k; g.n0 = n0; g.n = g.nf = q.batch / p.nsub + (k < q.batch % p.nsub ? 1 : 0); g.stream = k;
    n0 += g.n;
    g.scratch_off = (size_t)k * scratch_per; g.scratch_floats = scratch_per;
    g.stem = p.first_split == 0;
    Edge at = whole;
    const int rc = chain(g, p.first_split, nblocks, at);
    if (rc != ADX_OK) return rc;
  }
  return ADX_OK;
}

// Calls f(segment, i) for every step of segments seg[0 .. n) in issue order -- i = -1: the stem, 0 .. nsteps - 1: a block step,
// nsteps: the average pool + fc (sub-batches only) -- until one fails: layer by layer, alternating between the segments, so
// that every stream's queue has work early.  A forward is the prefix (if any) on its own, the fork, then the sub-batches together.
extern "C++" template <class F>
static int resnet_plan_each(const ResnetSegment* seg, int n, F&& f) {
  int rc = ADX_OK;
  for (int k = 0; k < n && rc == ADX_OK && seg[k].stem; ++k) rc = f(seg[k], -1);
  for (int i = 0; n > 0 && i < seg[0].nsteps + (seg[0].id > 0 ? 1 : 0); ++i)
    for (int k = 0; k < n && rc == ADX_OK; ++k) rc = f(seg[k], i);
  return rc;
}

int adx_resnet_plan_describe(const adx_resnet* r, int32_t batch, int32_t h, int32_t w, int32_t flags, int32_t* n_records, int32_t* ints,
                             int32_t max_records) {
  ADX_REQUIRE(r && n_records && ints, "adx_resnet_plan_describe: null argument");
  ADX_REQUIRE((flags & ~ADX_RESNET_PLAN_CAPTURING) == 0 && max_records >= 1, "adx_resnet_plan_describe: flags 0x%x, max_records %d",
              (unsigned)flags, max_records);
  ResnetEvalQuery q;
  q.batch = batch; q.h = h; q.w = w; q.capturing = (flags & ADX_RESNET_PLAN_CAPTURING) != 0;
  ResnetEvalPlan p;
  int rc = resnet_eval_plan(*r, q, &p);
  if (rc != ADX_OK) return rc;
  const ResnetLayout& lay = p.lay;
  int n = 0;
  // one launch: kind, block, conv, input map, output map, channels, kFmt* bits, buffers of x / residual / y / second output
  auto put = [&](const ResnetSegment& g, int kind, int block, int conv, int H, int W, int OH, int OW, int cin, int cout, int fmt, int x, int res,
                 int y, int y2, int status) {
    if (n < max_records) {
      const int32_t rec[ADX_RESNET_PLAN_INTS] = {g.id, g.stream, g.n0, g.n, g.nf, kind, block, conv, H, W, OH, OW, cin, cout, fmt, x, res, y, y2,
                                                 (int32_t)(g.scratch_off / 64), (int32_t)(g.scratch_floats / 64), status, p.nsub, p.first_split};
      memcpy(ints + (size_t)n * ADX_RESNET_PLAN_INTS, rec, sizeof(rec));
    }
    ++n;
  };
  auto record = [&](const ResnetSegment& g, int i) -> int {
    if (i < 0) {
      if (g.stem_fused) {
        put(g, ADX_RESNET_PLAN_STEM_POOL, -1, -1, h, w, lay.h2, lay.w2, 3, 64, g.pooled_cells ? kFmtYCells : 0, -1, -1, 0, -1, 0);
      } else {
        put(g, ADX_RESNET_PLAN_STEM, -1, -1, h, w, lay.h1, lay.w1, 3, 64, 0, -1, -1, kResnetBufStem, -1, 0);
        put(g, ADX_RESNET_PLAN_MAXPOOL, -1, -1, lay.h1, lay.w1, lay.h2, lay.w2, 64, 64, 0, kResnetBufStem, -1, 0, -1, 0);
      }
    } else if (i == g.nsteps) {
      put(g, ADX_RESNET_PLAN_AVGPOOL_FC, -1, -1, g.final_h, g.final_w, 1, 1, 512, r->out_dim, g.final_cells ? kFmtXCells : 0, g.final_buf, -1, -1,
          -1, 1 + (int)r->block_has_ds.size());
    } else {
      const ResnetBlockStep& t = g.steps[i];
      const ConvSpec& c1 = r->convs[t.c1];
      const int fmt1 = (t.in_cells ? kFmtXCells : 0) | (t.mid_cells ? kFmtYCells : 0);
      if (t.fused_ds) {
        put(g, ADX_RESNET_PLAN_ENTRY, t.block, 0, t.H, t.W, t.OH, t.OW, c1.cin, c1.cout, fmt1, t.in, -1, t.mid, t.id, t.status);
      } else {
        put(g, ADX_RESNET_PLAN_CONV, t.block, 0, t.H, t.W, t.OH, t.OW, c1.cin, c1.cout, fmt1, t.in, -1, t.mid, -1, t.status);
        if (r->block_has_ds[t.block]) put(g, ADX_RESNET_PLAN_CONV, t.block, 2, t.H, t.W, t.OH, t.OW, c1.cin, c1.cout, 0, t.in, -1, t.id, -1, t.status);
      }
      put(g, ADX_RESNET_PLAN_CONV, t.block, 1, t.OH, t.OW, t.OH, t.OW, c1.cout, c1.cout,
          (t.mid_cells ? kFmtXCells : 0) | (t.out_cells ? kFmtYCells : 0) | (t.id_cells ? kFmtResCells : 0), t.mid, t.id, t.out, -1, t.status);
    }
    return ADX_OK;
  };
  (void)resnet_plan_each(p.seg, p.nseg - p.nsub, record);
  (void)resnet_plan_each(p.seg + p.nseg - p.nsub, p.nsub, record);
  *n_records = n;
  ADX_REQUIRE(n <= max_records, "adx_resnet_plan_describe: %d launches, room for %d", n, max_records);
  return ADX_OK;
}

// The grids of the same plan's launches on a device of `cus` compute units: what conv2d_hs3x3_plan / conv2d_hs_s2_plan answer for
// every record of adx_resnet_plan_describe under the plan's reserve (the launch functions ask them the same question).
int adx_resnet_plan_grids(const adx_resnet* r, int32_t batch, int32_t h, int32_t w, int32_t flags, int32_t cus, int32_t reserve,
                          int32_t* n_records, int32_t* ints, int32_t max_records) {
  ADX_REQUIRE(r && n_records && ints, "adx_resnet_plan_grids: null argument");
  ADX_REQUIRE((flags & ~ADX_RESNET_PLAN_CAPTURING) == 0 && max_records >= 1 && cus >= 8, "adx_resnet_plan_grids: flags 0x%x, max_records %d, %d CUs",
              (unsigned)flags, max_records, cus);
  ResnetEvalQuery q;
  q.batch = batch; q.h = h; q.w = w; q.capturing = (flags & ADX_RESNET_PLAN_CAPTURING) != 0;
  ResnetEvalPlan p;
  const int rc = resnet_eval_plan(*r, q, &p);
  if (rc != ADX_OK) return rc;
  if (reserve >= 0) p.reserve_cus = reserve;        // (as ADX_HS_RESERVE_CUS pins it in resnet_eval_plan)
  const DebugSwitches& sw = debug_switches();
  const int usable = hs_usable_cus(cus, p.reserve_cus, sw.hs_grid_cap);
  int n = 0;
  auto put = [&](int persistent, int units, int slots, size_t grid) {
    if (n < max_records) {
      const int32_t rec[ADX_RESNET_GRID_INTS] = {persistent, units, slots, (int32_t)grid, p.reserve_cus, usable};
      memcpy(ints + (size_t)n * ADX_RESNET_GRID_INTS, rec, sizeof(rec));
    }
    ++n;
  };
  auto conv = [&](const ConvSpec& c, int nf, int H, int W, int fmt, bool has_res) {
    Hs3x3Query hq;
    hq.N = nf; hq.H = H; hq.W = W; hq.fmt = fmt; hq.affine = true; hq.relu = true; hq.has_res = has_res; hq.cus = usable;
    const Hs3x3Plan hp = c.k == 3 && c.stride == 1 ? conv2d_hs3x3_plan(c, hq, sw) : Hs3x3Plan{};
    if (hp.family == kHs3x3q) put(1, hp.cout_tiles * hp.tiles_x * hp.tiles_y, hp.q_slots, hp.grid);
    else put(0, 0, 0, hp.family == kHs3x3 ? hp.grid : 0);
  };
  auto record = [&](const ResnetSegment& g, int i) -> int {
    if (i < 0) {
      put(0, 0, 0, 0);
      if (!g.stem_fused) put(0, 0, 0, 0);
    } else if (i == g.nsteps) {
      put(0, 0, 0, 0);
    } else {
      const ResnetBlockStep& t = g.steps[i];
      const ConvSpec& c1 = r->convs[t.c1];
      if (t.fused_ds) {
        HsS2Query sq;
        sq.N = g.n; sq.H = t.H; sq.W = t.W; sq.x_cells = t.in_cells; sq.y_cells = t.mid_cells; sq.cus = usable;
        const HsS2Plan sp = conv2d_hs_s2_plan(c1, r->convs[t.c1 + 2], sq, sw);
        if (sp.q) put(1, sp.cout_tiles * sp.tiles_x * sp.tiles_y, sp.q_slots, sp.grid);
        else put(0, 0, 0, 0);
      } else {
        conv(c1, g.n, t.H, t.W, (t.in_cells ? kFmtXCells : 0) | (t.mid_cells ? kFmtYCells : 0), false);
        if (r->block_has_ds[t.block]) put(0, 0, 0, 0);
      }
      conv(r->convs[t.c1 + 1], g.n, t.OH, t.OW,
           (t.mid_cells ? kFmtXCells : 0) | (t.out_cells ? kFmtYCells : 0) | (t.id_cells ? kFmtResCells : 0), true);
    }
    return ADX_OK;
  };
  (void)resnet_plan_each(p.seg, p.nseg - p.nsub, record);
  (void)resnet_plan_each(p.seg + p.nseg - p.nsub, p.nsub, record);
  *n_records = n;
  ADX_REQUIRE(n <= max_records, "adx_resnet_plan_grids: %d launches, room for %d", n, max_records);
  return ADX_OK;
}

// The unit walk of conv2d_hs3x3q_kernel from the kernel's own range and unit functions (hs3x3q_walk, hs3x3q_unit; the stepping by Q
// is this function's copy of the kernel's loop, which the GPU bit-identity tests cover): workgroup b of `grid` visits counts[b]
// units; visits holds them workgroup after workgroup, in visiting order, as (spatial tile, cout tile) pairs.
int adx_conv2d_hs3x3q_walk(int32_t units, int32_t cout_tiles, int32_t grid, int32_t* counts, int32_t* visits) {
  ADX_REQUIRE(counts && visits && units >= 1 && cout_tiles >= 1 && units % cout_tiles == 0 && grid >= 8 && grid % 8 == 0,
              "adx_conv2d_hs3x3q_walk: %d units of %d cout tiles on %d workgroups", units, cout_tiles, grid);
  const int Q = grid / 8;
  int n = 0;
  for (int b = 0; b < grid; ++b) {
    const HsQWalk wk = hs3x3q_walk(b & 7, b >> 3, units);
    counts[b] = 0;
    for (int u = wk.first; u < wk.end; u += Q, ++counts[b], ++n) {
      ADX_REQUIRE(n < units, "adx_conv2d_hs3x3q_walk: internal error (more visits than units)");
      const HsQUnit un = hs3x3q_unit(u, cout_tiles);
      visits[2 * n] = un.sp;
      visits[2 * n + 1] = un.ct;
    }
  }
  return ADX_OK;
}

// The stage walk of conv2d_hs3x3_kernel's PAIR form over `nchunks` 16-channel chunks, from the tables the kernel's stage loop reads
// (hs_pair_stage, hs_pair_run); which stage fetches and writes what is this function's copy of that loop (prologue = stage -1),
// which the GPU tests cover.  Events of ADX_PAIR_EVENT_INTS words: include/adx.h.
int adx_conv2d_hs3x3_pair_walk(int32_t nchunks, int32_t* n_events, int32_t* events, int32_t max_events) {
  ADX_REQUIRE(n_events && events && nchunks >= 2 && nchunks % 2 == 0 && max_events >= 1, "adx_conv2d_hs3x3_pair_walk: %d chunks, room for %d events",
              nchunks, max_events);
  const int npairs = nchunks / 2, nstages = 9 * npairs;
  int n = 0;
  auto put = [&](int stage, int kind, int chunk, int tr, int cb, int rs, int idle) {
    if (n < max_events) {
      const int32_t e[ADX_PAIR_EVENT_INTS] = {stage, kind, chunk, tr, cb, rs, idle};
      memcpy(events + (size_t)n * ADX_PAIR_EVENT_INTS, e, sizeof(e));
    }
    ++n;
  };
  // prologue: stage 0's weights and the first chunk complete in LDS; stage 1's weights and chunk 1's first round in flight
  put(-1, ADX_PAIR_FETCH_W, -1, -1, -1, 0, 0);
  put(-1, ADX_PAIR_WRITE_W, -1, -1, 0, 0, 0);
  for (int k = 0; k < 3; ++k) { put(-1, ADX_PAIR_FETCH_P, 0, k, -1, -1, 0); put(-1, ADX_PAIR_WRITE_P, 0, k, 0, -1, 0); }
  put(-1, ADX_PAIR_FETCH_W, -1, -1, -1, 1, 0);
  put(-1, ADX_PAIR_FETCH_P, 1, 0, -1, -1, 0);
  for (int pair = 0; pair < npairs; ++pair)
    for (int i = 0; i < 9; ++i) {
      const int s = 9 * pair + i;
      const HsPairStage st = hs_pair_stage(i), nx = hs_pair_stage((i + 1) % 9);
      put(s, ADX_PAIR_FETCH_W, -1, -1, -1, s + 2 < nstages ? s + 2 : nstages - 1, s + 2 >= nstages);
      if (nx.pround >= 0) {
        const int c = 2 * pair + 1 + (i == 8 ? 2 : nx.pnext);
        put(s, ADX_PAIR_FETCH_P, c < nchunks ? c : nchunks - 1, nx.pround, -1, -1, c >= nchunks);
      }
      for (int t = 0; t < 2; ++t)
        put(s, ADX_PAIR_READ, 2 * pair + st.tap[t].odd, st.tap[t].kh * 3 + i % 3, st.tap[t].odd, hs_pair_run(pair, i, t) / 256, s & 1);
      put(s, ADX_PAIR_WRITE_W, -1, -1, (s + 1) & 1, s + 1 < nstages ? s + 1 : nstages - 1, s + 1 >= nstages);
      if (st.pround >= 0) {
        const int c = 2 * pair + 1 + st.pnext;
        put(s, ADX_PAIR_WRITE_P, c < nchunks ? c : nchunks - 1, st.pround, st.pnext ? 0 : 1, -1, c >= nchunks);
      }
    }
  *n_events = n;
  ADX_REQUIRE(n <= max_events, "adx_conv2d_hs3x3_pair_walk: %d events, room for %d", n, max_events);
  return ADX_OK;
}

// What conv2d_hs3x3_plan answers for a launch of this conv (no device needed): out = [family, tile mode, ksplit, PAIR form, admitted]
int adx_conv2d_hs3x3_plan_query(const adx_conv2d_desc* d, int32_t n, int32_t h, int32_t w, int32_t fmt, int32_t has_res, int32_t* out) {
  ConvSpec L;
  const int rc = spec_from_desc(d, &L);
  if (rc != ADX_OK) return rc;
  ADX_REQUIRE(out && n >= 1 && h >= 1 && w >= 1 && fmt >= 0 && fmt <= 7, "adx_conv2d_hs3x3_plan_query: n %d, %d x %d, fmt %d", n, h, w, fmt);
  Hs3x3Query q;
  q.N = n; q.H = h; q.W = w; q.fmt = fmt; q.affine = true; q.relu = true; q.has_res = has_res != 0; q.cus = 256;
  const Hs3x3Plan p = L.k == 3 && L.stride == 1 ? conv2d_hs3x3_plan(L, q) : Hs3x3Plan{};
  out[0] = p.family; out[1] = p.mode; out[2] = p.ksplit; out[3] = p.pair ? 1 : 0; out[4] = p.admitted ? 1 : 0;
  return ADX_OK;
}

static int resnet_forward_impl(adx_resnet* r, const void* packed, void* workspace, const float* img,
                               const uint8_t* frames_u8, const float* mean, const float* stdv, int32_t batch, int32_t h,
                               int32_t w, float* feature, adx_stream stream);

int adx_resnet_forward(adx_resnet* r, const void* packed, void* workspace, const float* img, int32_t batch, int32_t h,
                       int32_t w, float* feature, adx_stream stream) {
  ADX_REQUIRE(img != nullptr, "adx_resnet_forward: null image");
  return resnet_forward_impl(r, packed, workspace, img, nullptr, nullptr, nullptr, batch, h, w, feature, stream);
}

int adx_resnet_forward_u8(adx_resnet* r, const void* packed, void* workspace, const uint8_t* frames_hwc, const float* mean,
                          const float* stdv, int32_t batch, int32_t h, int32_t w, float* feature, adx_stream stream) {
  ADX_REQUIRE(frames_hwc && mean && stdv, "adx_resnet_forward_u8: null frames / mean / std");
  return resnet_forward_impl(r, packed, workspace, nullptr, frames_hwc, mean, stdv, batch, h, w, feature, stream);
}

// ADX_CHECK_RANGE=1 (debug): the split-fp16 kernels hold activations as fp16 hi / lo pairs, so a forward activation of
// |x| >= 65504 becomes inf and travels on silently ("Range").  In this mode every activation tensor of
// the perception pass is scanned right after the launch that wrote it and the call fails with the FIRST tensor that left
// the range (fp32 tensors: |x| >= 65504 or non-finite; cell tensors: a half with an all-ones exponent).  It synchronises
// the stream after every launch (no graph capture) and owns one device word.
__global__ void __launch_bounds__(256) range_scan_kernel(const uint32_t* __restrict__ v, size_t words, int cells, unsigned* flag) {
  bool bad = false;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) {
    const uint32_t b = v[i];
    if (cells) bad |= ((b & 0x7C00u) == 0x7C00u) | ((b & 0x7C000000u) == 0x7C000000u);
    else bad |= (b & 0x7FFFFFFFu) >= 0x477FE000u;            // 65504.0f
  }
  if (bad) atomicOr(flag, 1u);
}

extern "C++" int adx::conv2d_range_check(const char* what, int index, const float* t, size_t floats, bool cells, hipStream_t s) {
  if (!debug_switches().check_range) return ADX_OK;
  static unsigned* flag = nullptr;
  if (flag == nullptr) ADX_CHECK_HIP(hipMalloc(&flag, sizeof(unsigned)));
  ADX_CHECK_HIP(hipMemsetAsync(flag, 0, sizeof(unsigned), s));
  range_scan_kernel<<<dim3(1024), dim3(256), 0, s>>>(reinterpret_cast<const uint32_t*>(t), floats, cells ? 1 : 0, flag);
  ADX_LAUNCH_CHECK();
  unsigned h = 0;
  ADX_CHECK_HIP(hipMemcpyAsync(&h, flag, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  ADX_CHECK_HIP(hipStreamSynchronize(s));
  if (h != 0) {
    set_error("adx_resnet_forward: %s %d writes activations outside the fp16 range of the split kernels (|x| >= 65504 or "
              "non-finite); ADX_CONV_EXACT=1 runs the pass on the exact-fp32 kernels", what, index);
    return ADX_ERR_RANGE;
  }
  return ADX_OK;
}

// Carries out resnet_eval_plan: every decision between the fork and the join is the plan's.
static int resnet_forward_impl(adx_resnet* r, const void* packed, void* workspace, const float* img,
                               const uint8_t* frames_u8, const float* mean, const float* stdv, int32_t batch, int32_t h,
                               int32_t w, float* feature, adx_stream stream) {
  ADX_REQUIRE(r && packed && workspace && (img || frames_u8) && feature, "adx_resnet_forward: null argument");
  if (!r->packed_once) {
    set_error("adx_resnet_forward: weights were never packed (call adx_resnet_pack first)");
    return ADX_ERR_STATE;
  }
  hipStream_t s = (hipStream_t)stream;
  ResnetEvalQuery q;
  q.batch = batch; q.h = h; q.w = w; q.u8 = frames_u8 != nullptr;
  ResnetEvalPlan plan;
  int rc = resnet_eval_plan(*r, q, &plan);
  if (rc == ADX_OK && plan.nsub > 1) {      // (only a pass that would fork asks the runtime)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
      q.capturing = true;
      rc = resnet_eval_plan(*r, q, &plan);
    }
  }
  if (rc != ADX_OK) return rc;
  const int nsub = plan.nsub;
  if (nsub > 1) {
    int dev = 0;
    ADX_CHECK_HIP(hipGetDevice(&dev));
    if (r->side_device != dev || r->side[nsub - 2] == nullptr) {
      if (r->side_device != dev) {
        // the handle moved to another device (module.to(other_gpu)): streams AND events belong to the device they were
        // created on -- recording an old event on a new stream fails -- so all of them are recreated here
        for (auto& st : r->side) if (st != nullptr) { (void)hipStreamDestroy(st); st = nullptr; }
        if (r->ev_fork != nullptr) { (void)hipEventDestroy(r->ev_fork); r->ev_fork = nullptr; }
        for (auto& ev : r->ev_join) if (ev != nullptr) { (void)hipEventDestroy(ev); ev = nullptr; }
        r->side_device = dev;
      }
      if (r->ev_fork == nullptr) ADX_CHECK_HIP(hipEventCreateWithFlags(&r->ev_fork, hipEventDisableTiming));
      for (int k = 0; k < nsub - 1; ++k) {
        if (r->side[k] == nullptr) ADX_CHECK_HIP(hipStreamCreateWithFlags(&r->side[k], hipStreamNonBlocking));
        if (r->ev_join[k] == nullptr) ADX_CHECK_HIP(hipEventCreateWithFlags(&r->ev_join[k], hipEventDisableTiming));
      }
    }
  }

  const float* base = (const float*)packed;
  const ResnetLayout& lay = plan.lay;
  const int h1 = lay.h1, w1 = lay.w1, h2 = lay.h2, w2 = lay.w2;
  float* const ws = (float*)workspace;
  float* const region[4] = {ws + lay.stem, ws + lay.stem + lay.act, ws + lay.stem + 2 * lay.act, ws};
  // a segment's part of a buffer: from its first image's slot of the buffer's largest map
  auto at = [&](const ResnetSegment& g, int buf) { return region[buf] + (size_t)g.n0 * 64 * (buf == kResnetBufStem ? h1 * w1 : h2 * w2); };
  struct ScratchScope {     // split-reduction scratch of the 3x3 convs of THIS call
    void set(float* p, size_t n) { conv2d_set_split_scratch(p, n); }
    ~ScratchScope() { conv2d_set_split_scratch(nullptr, 0); }
  } scratch_scope;
  struct ReserveScope {     // the plan's reserve, for the persistent launches of THIS call
    explicit ReserveScope(int n) { conv2d_set_reserve_cus(n); }
    ~ReserveScope() { conv2d_set_reserve_cus(-1); }
  } reserve_scope(plan.reserve_cus);
  uint32_t* const words = r->status;      // range status (adx_resnet_set_status): [0] stem, [1 + b] block b, [1 + nblocks] fc
  StatusScope status_scope(words);

  auto issue = [&](const ResnetSegment& g, int i) -> int {
    hipStream_t st = g.stream == 0 ? s : r->side[g.stream - 1];
    const int n = g.n;
    scratch_scope.set(g.scratch_floats != 0 ? ws + g.scratch_off : nullptr, g.scratch_floats);
    int rc;
    if (i < 0) {                    // stem (+ pool)
      const ConvSpec& c0 = r->convs[0];
      const float* im = img != nullptr ? img + (size_t)g.n0 * 3 * h * w : nullptr;
      const uint8_t* fr = frames_u8 != nullptr ? frames_u8 + (size_t)g.n0 * 3 * h * w : nullptr;
      status_scope.set(words);
      float* pooled = at(g, 0);
      if (g.stem_fused) {
        rc = conv2d_hs_stem_pool(c0, im, base + c0.o_w, base + c0.o_scale, base + c0.o_shift, pooled, n, h, w, st, fr, mean, stdv,
                                 g.pooled_cells);
      } else {
        float* sm = at(g, kResnetBufStem);
        rc = conv2d_launch(c0, base, im, nullptr, sm, n, h, w, 1, st);
        if (rc != ADX_OK) return rc;
        rc = maxpool_launch(sm, pooled, n * 64, h1, w1, h2, w2, st);
      }
      if (rc != ADX_OK) return rc;
      return conv2d_range_check("the stem (conv1 + bn1 + relu + maxpool), tensor", 0, pooled, (size_t)n * 64 * h2 * w2, g.pooled_cells, st);
    }
    if (i == g.nsteps) {            // average pool + fc
      const int fc = 1 + (int)r->block_has_ds.size();
      return avgpool_fc_launch(at(g, g.final_buf), base + r->o_fcw, base + r->o_fcb, feature + (size_t)g.n0 * r->out_dim, n, 512,
                               g.final_h * g.final_w, r->out_dim, st, g.final_cells, words != nullptr ? words + fc : nullptr);
    }
    const ResnetBlockStep& t = g.steps[i];      // one BasicBlock
    const ConvSpec& c1 = r->convs[t.c1];
    const ConvSpec& c2 = r->convs[t.c1 + 1];
    status_scope.set(words != nullptr ? words + t.status : nullptr);
    const float* xin = at(g, t.in);
    float* mid = at(g, t.mid);
    float* identity = at(g, t.id);
    float* dst = at(g, t.out);
    if (t.fused_ds) {
      const ConvSpec& ds = r->convs[t.c1 + 2];
      rc = conv2d_hs_launch_block_s2(c1, ds, xin, base + c1.o_w, base + c1.o_scale, base + c1.o_shift, mid, base + ds.o_w, base + ds.o_scale,
                                     base + ds.o_shift, identity, n, t.H, t.W, st, t.in_cells, t.mid_cells);
      if (rc != ADX_OK) return rc;
    } else {
      rc = conv2d_launch(c1, base, xin, nullptr, mid, n, t.H, t.W, 1, st,            // conv1 + bn1 + relu
                         (t.in_cells ? kFmtXCells : 0) | (t.mid_cells ? kFmtYCells : 0));
      if (rc != ADX_OK) return rc;
      if (r->block_has_ds[t.block]) {
        rc = conv2d_launch(r->convs[t.c1 + 2], base, xin, nullptr, identity, n, t.H, t.W, 0, st);  // downsample conv + bn
        if (rc != ADX_OK) return rc;
      }
    }
    rc = conv2d_range_check("conv1 + bn1 + relu of BasicBlock", t.block, mid, (size_t)n * c1.cout * t.OH * t.OW, t.mid_cells, st);
    if (rc != ADX_OK) return rc;
    rc = conv2d_launch(c2, base, mid, identity, dst, n, t.OH, t.OW, 1, st,           // conv2 + bn2 + identity + relu
                       (t.mid_cells ? kFmtXCells : 0) | (t.out_cells ? kFmtYCells : 0) | (t.id_cells ? kFmtResCells : 0));
    if (rc != ADX_OK) return rc;
    return conv2d_range_check("the output of BasicBlock", t.block, dst, (size_t)n * c2.cout * t.OH * t.OW, t.out_cells, st);
  };

  rc = resnet_plan_each(plan.seg, plan.nseg - nsub, issue);
  if (nsub > 1) {
    ADX_CHECK_HIP(hipEventRecord(r->ev_fork, s));
    for (int k = 1; k < nsub; ++k) ADX_CHECK_HIP(hipStreamWaitEvent(r->side[k - 1], r->ev_fork, 0));
  }
  if (rc == ADX_OK) rc = resnet_plan_each(plan.seg + plan.nseg - nsub, nsub, issue);
  // join even after an error: a side stream must not be left forked from a capturing stream
  for (int k = 1; k < nsub; ++k) {
    if (hipEventRecord(r->ev_join[k - 1], r->side[k - 1]) == hipSuccess) (void)hipStreamWaitEvent(s, r->ev_join[k - 1], 0);
  }
  return rc;
}

}  // extern "C"
