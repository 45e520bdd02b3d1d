// fp32-equivalent conv2d on the fp16 matrix cores of gfx950 ("hs" = hi/lo split).
//
// gfx950 has no xf32/TF32 and its fp32 MFMA runs at the vector rate (157 TFLOP/s, 1/16 of the fp16/bf16
// rate), so an fp32-in/fp32-out convolution that wants the matrix cores' real throughput has to feed them
// 16-bit operands.  Every fp32 operand x (activation or weight) is split EXACTLY-ish into two fp16 numbers
//     hi = fp16(x)                     (round to nearest even, 11 significant bits)
//     lo = fp16((x - hi) * 2^11)       (the next 11 bits, scaled so it never falls into fp16 subnormals)
// so that x = hi + lo * 2^-11 up to a relative error of 2^-22 .. 2^-23, and a product is evaluated as
//     x * w  ~=  hi_x * hi_w  +  2^-11 * (hi_x * lo_w + lo_x * hi_w)
// (the dropped lo*lo term is 2^-22 relative).  fp16 x fp16 products are exact in the MFMA's fp32 datapath
// and both sums are accumulated in fp32 (two accumulators: `main` and `lo`, combined once in the epilogue),
// so the result carries a per-product error of ~7e-8 relative -- below the 1.6e-7 that an fp32 accumulation
// of the same length has on its own (measured: tests/test_gpu_ops.py::test_conv2d_hs_*).  It costs
// 3 x v_mfma_f32_32x32x16_f16 (16 k-values each, 32 cycles) where the exact-fp32 path needs
// 8 x v_mfma_f32_32x32x2_f32 (64 cycles each): 5.3x less matrix time, the same 4 bytes per operand in LDS.
// Range: |x| must stay below 65504 (fp16 max); larger values become inf/NaN loudly, and elements below 2^-14 keep
// an absolute (not relative) accuracy of 2^-36.  The ResNet's normalised image and batch-normalised activations
// are O(1..100).  Data gradients are not: the training executor hands their max|x| (Conv2dArgs::x_amax, computed
// by the kernel that produced them) and the kernel moves them into range by an exact power of two.
//
// Tile: one workgroup = 4 waves = 8 output rows x 32 output columns x 64 output channels; wave w owns rows
// 2w, 2w+1.  Per 16-channel chunk the input patch is split while it is staged (once per staged element) into
// LDS as [k-half][plane][pixel] 16-byte cells of 8 channels -- exactly the B fragment of one lane -- and the
// weight slab arrives pre-split from adx_*_pack as [tap][plane][k-half][cout] cells (the A fragment), so every
// operand read is one conflict-free ds_read_b128.  Global loads of the next stage are issued before the MFMAs
// of the current one and land in the other LDS buffer after them (one barrier per stage).  Epilogue as conv2d.hip: BN scale/shift, residual, ReLU, NCHW stores.
#include <type_traits>
#include <stdlib.h>

#include "adx_common.h"
#include "conv2d_internal.h"
#include "conv2d_hs_common.h"

namespace adx {

// Cell-layout store of one lane's 16 accumulator values of a 32-channel group (v[r]: channel (r & 3) + 8 (r >> 2) + 4 khalf
// of the lane's pixel; lane + 32 holds the other halves of the same cells).  Four v_permlane32_swap per pair of cells
// leave lanes 0-31 with cells 0 and 2 of the group and lanes 32-63 with cells 1 and 3, eight channels each (v[8 i + 0..7] =
// cell 2 i + khalf); then affine (sc / sh: LDS, indexed by the channel within the group's 64-channel slab), optional
// residual (res8[i]: the eight values of cell 2 i + khalf, or null), ReLU, split, two 16-byte stores per cell.
// so: SGPR byte offset of the group's first hi cell; cplane: bytes of one plane of cells; vcell: the lane's pixel * 16 +
// khalf * 2 * cplane, or the out-of-range offset.  amax: the lane's running maximum of |x| over the values it splits
// (adx_common.h: fp16_amax) at a pixel of the map (vcell in range): one select per call, not per value.
template <bool AFFINE = true>
__device__ __forceinline__ void cells_store32(float (&v)[16], const float* sc, const float* sh, int cl0, const float (*res8)[8],
                                              bool relu, __amdgpu_buffer_rsrc_t yrsrc, uint32_t vcell, uint32_t so, uint32_t cplane,
                                              float& amax) {
  float lm = 0.f;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const auto sw = __builtin_amdgcn_permlane32_swap(f2u(v[8 * i + j]), f2u(v[8 * i + 4 + j]), false, false);
      v[8 * i + j] = u2f(sw[0]);
      v[8 * i + 4 + j] = u2f(sw[1]);
    }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float t = AFFINE ? v[8 * i + j] * sc[cl0 + 16 * i + j] + sh[cl0 + 16 * i + j] : v[8 * i + j];
      if (res8 != nullptr) t += res8[i][j];
      o[j] = relu ? __builtin_fmaxf(t, 0.f) : t;
      lm = fp16_amax(lm, o[j]);
    }
    u32x4 hi, lo;
    split8(o, 1.f, hi, lo);
    const uint32_t sc2 = so + (uint32_t)(2 * i) * 2u * cplane;
    __builtin_amdgcn_raw_buffer_store_b128(hi, yrsrc, vcell, sc2, 0);
    __builtin_amdgcn_raw_buffer_store_b128(lo, yrsrc, vcell, sc2 + cplane, 0);
    // A VALU write to the data registers of a 16-byte buffer store in the next issue slot can reach the store (seen on
    // gfx950: one dword of ~1e-4 of the cells, run to run different); the compiler's hazard recogniser inserts the wait
    // state only for stores WITHOUT an SGPR offset, these have one.  The statement below keeps both data operands alive
    // across one wait state, wherever the scheduler puts it: nothing can write them before it.
    asm volatile("s_nop 0" ::"v"(hi), "v"(lo));
  }
  amax = fp16_amax(amax, vcell < 0xC0000000u ? lm : 0.f);
}

// STRIDE/K: the convolution; ROWS: output rows per wave (tile = 4*ROWS rows x 32 columns x 64 channels);
// PBUF: LDS copies of the patch (2: one barrier per stage; 1: an extra barrier per chunk, for the large stride-2
// patches); DS: also evaluate the BasicBlock's 1x1 stride-2 downsample conv (modeling/resnet.py:223-232) on the
// centre tap's operand fragments -- same input pixels, its own weights / BN / output tensor.
template <int STRIDE, int K, int ROWS, int PBUF, bool DS, bool XCELLS = false, bool YCELLS = false>
__global__ void __launch_bounds__(256, 2) conv2d_hs_kernel(const Conv2dArgs a) {
  static_assert(!DS || (K == 3 && STRIDE == 2 && PBUF == 1), "the fused downsample rides on the 3x3 stride-2 conv");
  constexpr int TH = 4 * ROWS;
  constexpr int PH = (TH - 1) * STRIDE + K;
  constexpr int PW = (kTileW - 1) * STRIDE + K;
  constexpr int EVW = (PW + 1) / 2;               // stride 2: a patch row is stored as [even columns][odd columns]
  constexpr int PLANE = PH * PW;                  // pixels of the staged patch
  constexpr int NITEM = 2 * PLANE;                // (k-half, pixel) cells per chunk
  constexpr int PIT = (NITEM + 255) / 256;
  constexpr int NTAPS = K * K;
  constexpr int NW = NTAPS * 256;                 // 16-byte weight cells per chunk: [tap][plane][k-half][64]
  constexpr int WST = K * 256;                    // weight cells of one stage (= one kernel row kh)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  u32x4* patch = reinterpret_cast<u32x4*>(smem_raw);   // PBUF x [k-half][plane][PLANE]
  u32x4* wl = patch + PBUF * 4 * PLANE;                // 2 x [kw][plane][k-half][64]
  u32x4* wds = wl + 2 * WST;                           // DS: [plane][k-half][64]
  float* ss = reinterpret_cast<float*>(wds + (DS ? 256 : 0));   // scale[64], shift[64] (+ the downsample's)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // workgroup -> tile: consecutive ids go to different XCDs (round robin), so give each XCD one contiguous
  // eighth of the tile space; neighbouring tiles (shared halos, shared weight slabs) then meet in one L2
  int bid = blockIdx.x;
  {
    const int per = gridDim.x >> 3;
    if (bid < per * 8) bid = (bid & 7) * per + (bid >> 3);
  }
  const int ct = bid % a.cout_tiles; bid /= a.cout_tiles;
  const int tx = bid % a.tiles_x; bid /= a.tiles_x;
  const int ty = bid % a.tiles_y; bid /= a.tiles_y;
  const int n = bid;
  const int oy0 = ty * TH, ox0 = tx * kTileW;
  const int iy0 = oy0 * STRIDE - a.pad, ix0 = ox0 * STRIDE - a.pad;
  const int cout0 = ct * kHsCout;
  const int l31 = lane & 31, khalf = lane >> 5;
  const size_t hw = (size_t)a.H * a.W;
  const float* xin = a.x + (size_t)n * a.Cin * hw;
  const int nchunks = a.cin_pad / kHsCC;
  const u32x4* wsrc = reinterpret_cast<const u32x4*>(a.w) + (size_t)ct * nchunks * NW;
  const u32x4* wdsrc = DS ? reinterpret_cast<const u32x4*>(a.w_ds) + (size_t)ct * nchunks * 256 : nullptr;

  // gather offset (bytes, from the chunk's first channel plane) of cell k's first channel.  The patch is read with
  // buffer loads: SGPR descriptor + 32-bit VGPR offset + SGPR channel offset (no 64-bit address math, PIT offset
  // registers in all), and cells outside the image use an offset beyond the descriptor's extent, which the
  // hardware range check turns into zeros -- the convolution's zero padding.
  constexpr uint32_t kOutside = 0xC0000000u;
  const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(xin), 0, (int)((size_t)a.Cin * hw * sizeof(float)), 0x00020000);
  const uint32_t plane_bytes = (uint32_t)(hw * sizeof(float));
  uint32_t goff[PIT];
  int pcell[PIT];        // LDS cell of item k inside its [k-half][plane] image
#pragma unroll
  for (int k = 0; k < PIT; ++k) {
    const int e = tid + 256 * k;
    const int hg = e >= PLANE ? 1 : 0;
    const int p = e - hg * PLANE;
    const int py = p / PW, px = p - py * PW;
    const int iy = iy0 + py, ix = ix0 + px;
    const bool ok = e < NITEM && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
    goff[k] = !ok ? kOutside
                  : XCELLS ? (uint32_t)(hg * 8 * hw * sizeof(float) + ((size_t)iy * a.W + ix) * 16)   // cell layout (conv2d_hs3x3_kernel)
                           : (uint32_t)((hg * 8 * hw + (size_t)iy * a.W + ix) * sizeof(float));
    pcell[k] = hg * 2 * PLANE + (STRIDE == 2 ? py * PW + (px & 1) * EVW + (px >> 1) : p);
  }
  if (tid < 2 * kHsCout) {
    const int c = cout0 + (tid & (kHsCout - 1));
    ss[tid] = a.scale == nullptr ? (tid < kHsCout ? 1.f : 0.f) : (tid < kHsCout ? a.scale[c] : a.shift[c]);
    if (DS) ss[2 * kHsCout + tid] = a.scale_ds == nullptr ? (tid < kHsCout ? 1.f : 0.f) : (tid < kHsCout ? a.scale_ds[c] : a.shift_ds[c]);
  }

  // optional dynamic range: scale x so that max|x| lands in [2^14, 2^15), undone exactly in the epilogue
  float xs = 1.f, xs_inv = 1.f;
  if (a.x_amax != nullptr) {
    uint32_t* red = reinterpret_cast<uint32_t*>(ss + (DS ? 4 : 2) * kHsCout);
    uint32_t b = 0;
    for (int i = tid; i < a.x_amax_n; i += 256) b = a.x_amax[i] > b ? a.x_amax[i] : b;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)b, off, 64);
      b = o > b ? o : b;
    }
    if (lane == 0) red[wave] = b;
    __syncthreads();
    b = red[0] > red[1] ? red[0] : red[1];
    b = red[2] > b ? red[2] : b;
    b = red[3] > b ? red[3] : b;
    const int e = (int)((b >> 23) & 0xFF);
    if (e != 0 && e != 255) {
      int sh = 127 + 14 - e;
      sh = sh > 100 ? 100 : (sh < -100 ? -100 : sh);
      xs = __builtin_bit_cast(float, (uint32_t)(127 + sh) << 23);
      xs_inv = __builtin_bit_cast(float, (uint32_t)(127 - sh) << 23);
    }
  }

  constexpr int NDS = DS ? ROWS : 0;
  f32x16 accm[ROWS][2], accl[ROWS][2];   // [row][cout half]: hi*hi sums, cross-term sums (scaled by 2^11)
  f32x16 adm[NDS + 1][2], adl[NDS + 1][2];
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        accm[r][m][i] = 0.f; accl[r][m][i] = 0.f;
        if (DS) { adm[r][m][i] = 0.f; adl[r][m][i] = 0.f; }
      }

  // Pipeline stage = (chunk, kernel row kh): weights are double-buffered per stage, the patch per chunk, so one
  // barrier per stage is enough and only K weight cells + PIT patch cells per thread are ever in registers.
  float pv[(PIT == K && PBUF == 2) ? 1 : PIT][8];
  u32x4 wv[K];
  u32x4 wdv;
  // the patch of the next chunk travels in K slices, one per stage (round k of the cell list <-> stage kh), so only
  // one slice (8 registers) is in flight at a time; with PIT != K everything goes with the first stage
  constexpr bool kSliced = (PIT == K) && PBUF == 2;
  auto load_p = [&](int chunk, int k0, int k1) {
    const uint32_t cbase = (uint32_t)chunk * kHsCC * plane_bytes;
#pragma unroll
    for (int k = k0; k < k1; ++k) {
      if (XCELLS) {
        const u32x4 h4 = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, goff[k], cbase, 0);
        const u32x4 l4 = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, goff[k], cbase + 4 * plane_bytes, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          pv[kSliced ? 0 : k][j] = u2f(h4[j]);
          pv[kSliced ? 0 : k][4 + j] = u2f(l4[j]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          pv[kSliced ? 0 : k][j] =
              __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, goff[k], cbase + j * plane_bytes, 0));
      }
    }
    if (DS && k0 == 0) wdv = wdsrc[(size_t)chunk * 256 + tid];
  };
  auto store_p = [&](int buf, int k0, int k1) {
    u32x4* pd = patch + buf * 4 * PLANE;
#pragma unroll
    for (int k = k0; k < k1; ++k) {
      const int e = tid + 256 * k;
      if (PIT * 256 == NITEM || e < NITEM) {
        u32x4 hi, lo;
        if (XCELLS) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            hi[j] = __builtin_bit_cast(uint32_t, pv[kSliced ? 0 : k][j]);
            lo[j] = __builtin_bit_cast(uint32_t, pv[kSliced ? 0 : k][4 + j]);
          }
        } else {
          split8(pv[kSliced ? 0 : k], xs, hi, lo);
        }
        pd[pcell[k]] = hi;
        pd[pcell[k] + PLANE] = lo;
      }
    }
    if (DS && k0 == 0) wds[tid] = wdv;
  };
  auto load_w = [&](int stage) {
    const u32x4* ws = wsrc + (size_t)stage * WST;
#pragma unroll
    for (int k = 0; k < K; ++k) wv[k] = ws[tid + 256 * k];
  };
  auto store_w = [&](int buf) {
#pragma unroll
    for (int k = 0; k < K; ++k) wl[buf * WST + tid + 256 * k] = wv[k];
  };

  const int pb_lane = khalf * 2 * PLANE + (wave * ROWS * STRIDE) * PW + (STRIDE == 2 ? l31 : l31 * STRIDE);
  const int wa_lane = khalf * 64 + l31;
  const int nstages = nchunks * K;

  load_w(0);
  store_w(0);
  if (kSliced) {
#pragma unroll
    for (int k = 0; k < PIT; ++k) { load_p(0, k, k + 1); store_p(0, k, k + 1); }
  } else {
    load_p(0, 0, PIT);
    store_p(0, 0, PIT);
  }
  __syncthreads();
  struct Frags { f16x8 A[2][2], B[2][ROWS]; };   // [plane][cout half], [plane][row]
  int stage = 0;
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    const u32x4* pb0 = patch + (PBUF == 2 ? (chunk & 1) * 4 * PLANE : 0) + pb_lane;
#pragma unroll
    for (int kh = 0; kh < K; ++kh, ++stage) {
      const u32x4* wa0 = wl + (stage & 1) * WST + wa_lane;
      if (stage + 1 < nstages) load_w(stage + 1);
      if (chunk + 1 < nchunks) {
        if (kSliced) load_p(chunk + 1, kh, kh + 1);
        else if (kh == 0) load_p(chunk + 1, 0, PIT);
      }
      auto fetch = [&](Frags& f, int kw) {
        const int col = STRIDE == 2 ? (kw & 1) * EVW + (kw >> 1) : kw;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
          for (int m = 0; m < 2; ++m) f.A[pl][m] = __builtin_bit_cast(f16x8, wa0[(kw * 2 + pl) * 128 + m * 32]);
#pragma unroll
          for (int r = 0; r < ROWS; ++r) f.B[pl][r] = __builtin_bit_cast(f16x8, pb0[pl * PLANE + (r * STRIDE + kh) * PW + col]);
        }
      };
      Frags fr[2];               // fragments of tap kw+1 are fetched under the MFMAs of tap kw
      fetch(fr[0], 0);
#pragma unroll
      for (int kw = 0; kw < K; ++kw) {
        const Frags& f = fr[kw & 1];
        if (kw + 1 < K) fetch(fr[(kw + 1) & 1], kw + 1);
        __builtin_amdgcn_sched_barrier(0);     // the next tap's reads are issued before this tap's MFMAs, in this order
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
#pragma unroll
          for (int m = 0; m < 2; ++m) {
            accm[r][m] = hs_mfma(f.A[0][m], f.B[0][r], accm[r][m]);
            accl[r][m] = hs_mfma(f.A[0][m], f.B[1][r], accl[r][m]);
            accl[r][m] = hs_mfma(f.A[1][m], f.B[0][r], accl[r][m]);
          }
        if (DS && kh == 1 && kw == 1) {   // x[2 oy][2 ox]: the 1x1 stride-2 conv's only tap
          f16x8 D[2][2];
#pragma unroll
          for (int pl = 0; pl < 2; ++pl)
#pragma unroll
            for (int m = 0; m < 2; ++m) D[pl][m] = __builtin_bit_cast(f16x8, wds[pl * 128 + wa_lane + m * 32]);
#pragma unroll
          for (int r = 0; r < ROWS; ++r)
#pragma unroll
            for (int m = 0; m < 2; ++m) {
              adm[r][m] = hs_mfma(D[0][m], f.B[0][r], adm[r][m]);
              adl[r][m] = hs_mfma(D[0][m], f.B[1][r], adl[r][m]);
              adl[r][m] = hs_mfma(D[1][m], f.B[0][r], adl[r][m]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (stage + 1 < nstages) store_w((stage + 1) & 1);
      if (chunk + 1 < nchunks) {
        if (kSliced) {
          store_p((chunk + 1) & 1, kh, kh + 1);
        } else if (kh == K - 1) {
          if (PBUF == 1) __syncthreads();      // every wave is done with the only patch copy
          store_p(PBUF == 2 ? (chunk + 1) & 1 : 0, 0, PIT);
        }
      }
      __syncthreads();
    }
  }

  // ---- epilogue: combine, BN scale/shift, residual, ReLU; lane = pixel column, register = channel ----
  // All residual loads of the tile are issued up front (the staging registers are dead by now): one exposed
  // latency per tile instead of one per 16 values.
  // Buffer descriptors: one instruction per access (wave-uniform channel offset in an SGPR, the lane's pixel in one
  // 32-bit VGPR); lanes outside the map carry the out-of-range offset (loads return 0, stores are dropped); without a
  // residual the descriptor is empty and every load returns 0.
  const int ox = ox0 + l31;
  // plain store: channel cout0 + c of an OH x OW map.  Depth-to-space store (Conv2dArgs::d2s_cin): this workgroup's 64
  // channels belong to ONE parity class (d2s_cin is a multiple of 64), i.e. to channels ci0 .. ci0 + 63 of a d2s_h x d2s_w map
  // at the pixels (2 oy + py, 2 ox + px)
  const bool d2s = !DS && a.d2s_cin > 0;
  const int cls = d2s ? cout0 / a.d2s_cin : 0, py = cls >> 1, px = cls & 1;
  const int sH = d2s ? a.d2s_h : a.OH, sW = d2s ? a.d2s_w : a.OW, sC = d2s ? a.d2s_cin : a.Cout;
  const uint32_t plane_ob = (uint32_t)(sH * sW) * (uint32_t)sizeof(float);
  const size_t img = (size_t)n * sC * sH * sW;
  const int img_bytes = (int)(sC * plane_ob);
  constexpr uint32_t kOut = 0xC0000000u;
  const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(a.y + img, 0, img_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t drsrc = __builtin_amdgcn_make_buffer_rsrc(DS ? a.y_ds + img : a.y, 0, DS ? img_bytes : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rrsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.res != nullptr ? a.res + img : a.y), 0, a.res != nullptr ? img_bytes : 0, 0x00020000);
  const uint32_t cbase_o = (uint32_t)(d2s ? cout0 - cls * a.d2s_cin : cout0) * plane_ob;
  if constexpr (YCELLS) {
    // both outputs as cell tensors (conv2d_hs3x3_kernel reads them: conv2 of the block takes y as its input and y_ds as its
    // residual); no residual and no depth-to-space store on this path (the host checks)
    const uint32_t cplane = (uint32_t)(a.OH * a.OW) * 16u;
    const uint32_t cell0 = (uint32_t)(cout0 >> 3) * 2u * cplane;
    float amax = 0.f;
#pragma unroll
    for (int rr = 0; rr < ROWS; ++rr) {
      const int oy = oy0 + wave * ROWS + rr;
      const uint32_t vcell = (oy < a.OH && ox < a.OW) ? (uint32_t)(oy * a.OW + ox) * 16u + (uint32_t)khalf * 2u * cplane : kOut;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        float v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = (accm[rr][half][r] + accl[rr][half][r] * (1.f / kLoScale)) * xs_inv;
        cells_store32(v, ss, ss + kHsCout, half * 32 + 8 * khalf, nullptr, a.relu != 0, yrsrc, vcell,
                      cell0 + (uint32_t)(half * 4) * 2u * cplane, cplane, amax);
        if (DS) {
#pragma unroll
          for (int r = 0; r < 16; ++r) v[r] = (adm[rr][half][r] + adl[rr][half][r] * (1.f / kLoScale)) * xs_inv;
          cells_store32(v, ss + 2 * kHsCout, ss + 3 * kHsCout, half * 32 + 8 * khalf, nullptr, false, drsrc, vcell,
                        cell0 + (uint32_t)(half * 4) * 2u * cplane, cplane, amax);
        }
      }
    }
    range_flag(a.status, out_of_fp16(amax));
    return;
  }
  uint32_t voff[ROWS];
#pragma unroll
  for (int rr = 0; rr < ROWS; ++rr) {
    const int oy = oy0 + wave * ROWS + rr;
    const int yy = d2s ? 2 * oy + py : oy, xx = d2s ? 2 * ox + px : ox;
    voff[rr] = (oy < a.OH && ox < a.OW && yy < sH && xx < sW) ? (uint32_t)(yy * sW + xx) * 4u + (uint32_t)(4 * khalf) * plane_ob : kOut;
  }
  float rv[ROWS][2][16];
#pragma unroll
  for (int rr = 0; rr < ROWS; ++rr)
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cu = half * 32 + (r & 3) + 8 * (r >> 2);     // + 4 * khalf, which rides in voff
        rv[rr][half][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rrsrc, voff[rr], cbase_o + cu * plane_ob, 0));
      }
  float amax = 0.f;         // range status (adx_common.h: fp16_amax)
#pragma unroll
  for (int rr = 0; rr < ROWS; ++rr) {
    float lm = 0.f;        // this row's values; only a pixel of the map counts
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cu = half * 32 + (r & 3) + 8 * (r >> 2);
        const int cl = cu + 4 * khalf;
        float v = (accm[rr][half][r] + accl[rr][half][r] * (1.f / kLoScale)) * xs_inv;
        v = v * ss[cl] + ss[kHsCout + cl];
        v += rv[rr][half][r];
        if (a.relu) v = v > 0.f ? v : 0.f;
        lm = fp16_amax(lm, v);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), yrsrc, voff[rr], cbase_o + cu * plane_ob, 0);
        if (DS) {    // downsample branch: BN only (resnet.py:230-231), no ReLU, no residual
          const float d = (adm[rr][half][r] + adl[rr][half][r] * (1.f / kLoScale)) * xs_inv;
          const float dv = d * ss[2 * kHsCout + cl] + ss[3 * kHsCout + cl];
          lm = fp16_amax(lm, dv);
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, dv), drsrc, voff[rr], cbase_o + cu * plane_ob, 0);
        }
      }
    amax = fp16_amax(amax, voff[rr] != kOut ? lm : 0.f);
  }
  range_flag(a.status, out_of_fp16(amax));
}

// ---- 3x3 stride-1, deferred-store pipeline ---------------------------------------------------------------------
// Same LDS images and arithmetic as conv2d_hs_kernel<1,3,2,2,false>; what changes is WHEN staged data moves and how
// much of it a CU needs per MFMA.
//  * There the loads of stage s+1 are issued at the start of stage s and converted + written to LDS after its MFMAs,
//    so every stage ends with a serial tail (wait for HBM, ~60 VALU, 5 LDS writes, LDS drain, barrier).  Here data is
//    fetched TWO stages ahead into a second register set, and the set that arrived during the previous stage is split
//    and written between the MFMAs of this stage; a stage ends with just the LDS drain and the barrier.  Two chunks
//    (6 stages) are unrolled so that every register-set index is a constant, and the stage body has no branches:
//    with control flow the compiler's s_waitcnt bookkeeping merges states and every wait degrades to vmcnt(0).
//  * Measured on the 4-wave tile (SQ counters, tools/pmc_sq.sh; 512->512 layer): SQ_VALU_MFMA_BUSY 53 % at an
//    effective 1.98 GHz, i.e. ~1040 TFLOP/s of fp16 MFMA; ONE workgroup per CU is as fast as two, removing the LDS
//    fragment reads changes 7 %, and tiles that move 18-35 % fewer operand bytes per MFMA (MODE 1 / 2) change
//    nothing: the loop runs at the MFMA rate the chip sustains on random data (MI355X_MICROARCH.md quotes 1247
//    TFLOP/s for a tuned bf16 GEMM at 1.9-1.95 GHz), not at a rate set by operand delivery.  With all-zero operands
//    the same launches are 22-25 % faster (ZERO=1 tools/bench_conv.py): the limit is power, i.e. data-dependent
//    clock-down, and what shortens a launch is fewer MFMAs / instructions / bytes, not fewer stalls.  Tile modes:
//      MODE 0: 4 waves,  8 rows x 32 columns x  64 channels (two per CU)  19.5 KB per 36 MFMAs/wave
//      MODE 1: 8 waves, 16 rows x 32 columns x  64 channels               25.4 KB per 2 x 36   (-35 %)
//      MODE 2: 8 waves,  8 rows x 32 columns x 128 channels               31.9 KB per 2 x 36   (-18 %; 8-row maps)
#ifdef ADX_HS_TRACE
// diagnostic build (-DADX_HS_TRACE): every workgroup of conv2d_hs3x3_kernel leaves the shader clock at its phase
// boundaries and the hardware slot it ran on; tools/hs_trace.py reads them back through adx_hs_trace_read
__device__ unsigned long long g_hs_trace[8 * 16384];
__device__ __forceinline__ void hs_trace(int slot) {
  if (threadIdx.x == 0 && blockIdx.x < 16384) g_hs_trace[blockIdx.x * 8 + slot] = __builtin_readcyclecounter();
}
__device__ __forceinline__ void hs_trace_id() {
  if (threadIdx.x == 0 && blockIdx.x < 16384) {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    g_hs_trace[blockIdx.x * 8 + 7] = ((unsigned long long)xcc << 32) | hw;
  }
}
#define HS_TRACE(slot) hs_trace(slot)
#else
#define HS_TRACE(slot)
#endif

// XCELLS / YCELLS: the input / output tensor is in the CELL layout instead of fp32 NCHW -- per image [C / 8][plane: hi, lo][H][W]
// cells of 16 bytes = the 8 channels of one pixel already split into fp16 hi / lo, i.e. exactly what the staging writes to
// LDS.  Same bytes per tensor, but the consumer's staging is two 16-byte loads + two LDS writes per cell pair where the fp32
// layout costs eight 4-byte loads and ~48 VALU instructions, once per 64-channel output slab; the producer splits each
// element once.  The products are bit-identical either way (the halves are the ones the consumer would have computed); a
// residual read from cells (Conv2dArgs::res_cells) is hi + lo / 2^11, the tensor to 2^-23.  Inference executor only.
// STATS: 0 none; 1 the training forward's BatchNorm statistics of this conv's own output; 2 (data-gradient launches) the
// BACKWARD sums of the BatchNorm in front of this conv in forward order, whose incoming gradient this launch produces
// (Conv2dArgs::bs_*).
// VR: the column tiles run over the virtual row of the whole batch (below) although the OUTPUT is fp32 NCHW -- the training
// forward and data-gradient launches (round 5): a map 225 / 113 / 57 / 29 columns wide pays one padded MFMA column per image
// instead of the round-up to 32, like the cell launches; YCELLS implies it.
// PAIR (MODE 0, STATS 0): the same tile, patch images and packed weights on v_mfma_f32_16x16x32_f16 -- K = 32 is TWO TAPS x the
// 16 channels of a chunk (conv2d_internal.h: hs_pair_stage), so the patch copies stay what MODE 0 stages (a 32-channel chunk
// would double them: conv2d_hs16.hip needs 8 waves and a whole CU for that) and a stage's weights are two 256-cell runs, 16 KB
// double-buffered: 60 KB, two workgroups per CU as before.  Lane (j = lane & 15, kq = lane >> 4), kq = (tap of the stage's
// pair, k-half of the chunk): the B fragment of pixel block pb is the cell of the lane's tap and k-half at row pb >> 1, column
// 16 (pb & 1) + j -- from the patch copy of that tap's chunk, a per-lane base where the two taps come from different chunks --
// and the A fragment of channel block cb the cell tap * 256 + plane * 128 + k-half * 64 + 16 cb + j of the stage's buffer.  The
// two k-groups that share a ds_read_b128 lane group (MI355X: lanes 0-3, 12-15, 20-27 | ...) differ in the k-half only.  Their
// weight cells lie 64 cells apart (0 mod 16: complementary banks, conflict-free).  Their patch cells lie one k-half of a patch copy
// apart: at the 32x32x16 form's pitch of 2 PLANE = 680 cells, 8 mod 16, lanes 20-27 (columns 4-11 of the second k-half) fell on the
// banks of lanes 0-3 and 12-15 and every patch read was 2-way (SQ_LDS_BANK_CONFLICT: a quarter of the launch's LDS cycles,
// profiles/README.md).  So the PAIR instantiations pitch the k-halves kHsPairKHalf = 688 cells apart, the next multiple of 16: columns
// 4-11 of the second k-half take the banks columns 0-3 and 12-15 of the first leave free; 16 cells = 256 bytes more per copy.
// Wave tile 64 channels x (2 rows x 32 columns) as 4 x 4 blocks of 16 x 16: 16 fragment reads and 48 MFMAs per stage; the
// products and their order per accumulator as in conv2d_hs3x3q_kernel.
constexpr int kHsPairKHalf = 688;
static_assert(kHsPairKHalf % 16 == 0 && kHsPairKHalf >= 2 * 10 * 34, "the k-half pitch of the PAIR form: whole bank rounds, two planes");
template <int MODE, int STATS = 0, bool XCELLS = false, bool YCELLS = false, bool VR = false, bool PAIR = false>
__global__ void __launch_bounds__(MODE == 0 ? 256 : 512, 2) conv2d_hs3x3_kernel(const Conv2dArgs a) {
  static_assert(!PAIR || (MODE == 0 && STATS == 0), "the PAIR form is the plain 4-wave tile");
  constexpr bool VROW = YCELLS || VR;
  constexpr int NT = MODE == 0 ? 256 : 512;            // threads
  constexpr int TH = MODE == 1 ? 16 : 8;               // output rows per workgroup
  constexpr int CT = MODE == 2 ? 2 : 1;                // 64-channel slabs per workgroup
  constexpr int K = 3, PH = TH + 2, PW = 34, PLANE = PH * PW, NITEM = 2 * PLANE;
  // cell pitch of a k-half ([hi plane][lo plane]) and of a patch copy (two k-halves); PAIR: kHsPairKHalf, 0 mod 16 (above)
  constexpr int KHP = PAIR ? kHsPairKHalf : 2 * PLANE, COPY = 2 * KHP;
  static_assert(KHP >= 2 * PLANE, "a k-half holds its two planes");
  constexpr int PIT = (NITEM + NT - 1) / NT;           // patch rounds = slices, one per stage while they last
  constexpr int NW = 9 * 256, WST = PAIR ? 2 * 256 : 3 * 256 * CT;      // weight cells per chunk and 64-channel slab / per stage
  constexpr int WIT = (WST + NT - 1) / NT;
  static_assert(PIT <= K, "a patch slice travels with each stage of a chunk");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  u32x4* patch = reinterpret_cast<u32x4*>(smem_raw);   // 2 x [k-half][plane][PLANE]
  u32x4* wl = patch + 2 * COPY;                   // 2 x [slab][kw][plane][k-half][64]
  float* ss = reinterpret_cast<float*>(wl + 2 * WST);  // scale[64 CT], shift[64 CT], 8 words for the range reduction
  u32x4* dummy = reinterpret_cast<u32x4*>(ss + 2 * 64 * CT + 8);   // where idle threads of a partial round write
  float* bsl = reinterpret_cast<float*>(dummy + 3);                 // STATS == 2: [mean | rstd | mask scale | mask shift] x 64 CT
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rowpair = MODE == 2 ? (wave & 3) : wave, slab = MODE == 2 ? (wave >> 2) : 0;
#ifdef ADX_HS_TRACE
  hs_trace_id();
#endif
  HS_TRACE(0);
  int bid = blockIdx.x;
  {
    const int per = gridDim.x >> 3;
    if (bid < per * 8) bid = (bid & 7) * per + (bid >> 3);
  }
  int kpart = 0;                       // split reduction (Conv2dArgs::ksplit): this workgroup's share of the chunks
  if (a.ksplit > 1) { kpart = bid % a.ksplit; bid /= a.ksplit; }
  const int ct = bid % a.cout_tiles; bid /= a.cout_tiles;
  const int tx = bid % a.tiles_x; bid /= a.tiles_x;
  const int ty = bid % a.tiles_y; bid /= a.tiles_y;
  const int n = VROW ? 0 : bid;
  const int oy0 = ty * TH, ox0 = tx * kTileW;
  const int iy0 = oy0 - a.pad, ix0 = ox0 - a.pad;
  const int cout0 = (ct * CT + slab) * kHsCout;
  const int l31 = lane & 31, khalf = lane >> 5;
  // YCELLS (the inference executor's launches): column tiles run over a VIRTUAL row -- the images of the batch side by side,
  // vw = W + 1 columns each: the W real ones and ONE all-zero column, which is the right padding of its image and the left
  // padding of the next one (pad = 1) -- so a map 225 / 113 / 57 / 29 wide pays one padded MFMA column per image instead of
  // 31 / 15 / 7 / 3: 452 tiles instead of 512 per tile row at B = 64.  The staged patch row is the 34 consecutive virtual
  // columns around the tile, whatever images they belong to, and the lane of virtual column v reads cell (lane + kw) exactly
  // as in the per-image tiling: consecutive lanes, consecutive 16-byte cells, no bank conflict.  (Round 3 gave every image
  // segment of a tile its own two halo cells, i.e. lanes behind an image boundary read two cells further: a 2-way conflict in
  // nearly every 16-lane group of a tile that holds a boundary -- 25 % of the LDS cycles of the 512-channel layers.)
  const int vx0 = tx * kTileW;
  const int ecol = PAIR ? 16 * ((lane >> 4) & 1) + (lane & 15) : l31;      // the tile column this lane's epilogue stores
  const int vl = vx0 + ecol;
  auto vdiv = [&](int v) { return (int)(((float)v + 0.5f) * a.inv_vw); };     // v / vw for 0 <= v < 2^21 (launch check)
  const int nl = VROW ? vdiv(vl) : 0, xl = VROW ? vl - nl * a.vw : 0;
  const bool lane_valid = !VROW || (nl < a.N && xl < a.W);
  const size_t hw = (size_t)a.H * a.W;
  const int nchunks_all = a.cin_pad / kHsCC;
  const int nchunks = a.ksplit > 1 ? a.cper : nchunks_all;       // chunks THIS workgroup reduces over
  const int chunk0 = kpart * nchunks;
  const float* xin = a.x + ((size_t)n * a.Cin + (size_t)chunk0 * kHsCC) * hw;      // YCELLS: n = 0, chunk0 = 0: the whole tensor
  const int nstages = nchunks * K;
  const u32x4* wsrc = reinterpret_cast<const u32x4*>(a.w) + ((size_t)ct * CT * nchunks_all + chunk0) * NW;
  constexpr uint32_t kOutside = 0xC0000000u;
  const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(xin), 0,
      (int)(uint32_t)((VROW ? (size_t)a.N * a.Cin : (size_t)(a.Cin - chunk0 * kHsCC)) * hw * sizeof(float)), 0x00020000);
  const uint32_t plane_bytes = (uint32_t)(hw * sizeof(float));
  uint32_t goff[PIT];
  int pcell[PIT];
#pragma unroll
  for (int k = 0; k < PIT; ++k) {
    const int e = tid + NT * k;
    const int hg = e >= PLANE ? 1 : 0;
    const int p = e - hg * PLANE;
    const int py = p / PW, px = p - py * PW;
    const int iy = iy0 + py;
    int ix = ix0 + px, ni = n;
    if constexpr (VROW) {          // patch column px = virtual column vx0 - 1 + px -> (image, input column); column W of an image is zero
      const int v = vx0 - 1 + px;
      ni = vdiv(v < 0 ? 0 : v);
      ix = v - ni * a.vw;          // -1 for the column left of the first image
    }
    const bool ok = e < NITEM && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W && ni < a.N;
    const size_t ioff = VROW ? (size_t)ni * a.Cin * hw * sizeof(float) : 0;
    goff[k] = !ok ? kOutside
                  : XCELLS ? (uint32_t)(ioff + hg * 8 * hw * sizeof(float) + ((size_t)iy * a.W + ix) * 16)   // cell (2 chunk + hg, hi, iy, ix)
                           : (uint32_t)(ioff + (hg * 8 * hw + (size_t)iy * a.W + ix) * sizeof(float));
    pcell[k] = e < NITEM ? hg * KHP + p : -1;
  }
  // weight cells of this thread: global offset inside a stage (slab-major) and LDS cell, or the dummy
  int wsrc_off[WIT], wdst[WIT];
#pragma unroll
  for (int k = 0; k < WIT; ++k) {
    const int e = tid + NT * k;
    const int sl = e / 768, within = e - sl * 768;
    const bool ok = e < WST;
    wsrc_off[k] = ok ? sl * nchunks_all * NW + within : 0;
    wdst[k] = ok ? e : -1;
  }
  // BN scale / shift of this workgroup's channels: requested now, parked in LDS after the first stage's data (a wait
  // here would put one more memory round trip in front of the first patch load)
  float ssv = 0.f;
  if (tid < 2 * 64 * CT) {
    const int half = tid / (64 * CT), cc = tid - half * 64 * CT;
    const int c = ct * CT * kHsCout + cc;
    ssv = a.scale == nullptr ? (half == 0 ? 1.f : 0.f) : (half == 0 ? a.scale[c] : a.shift[c]);
  }
  float bsv = 0.f;
  if (STATS == 2 && tid < 4 * 64 * CT) {
    const int which = tid / (64 * CT), cc = tid - which * 64 * CT;
    const int c = ct * CT * kHsCout + cc;
    // the mask's affine form exactly as the forward pass applied it (resnet_train.hip: bn_affine)
    const float mu = a.bs_mean[c], rs = a.bs_rstd[c];
    const float sc = a.bs_gamma[c] * rs;
    bsv = which == 0 ? mu : (which == 1 ? rs : (which == 2 ? sc : __builtin_fmaf(-mu, sc, a.bs_beta[c])));
  }
  float xs = 1.f, xs_inv = 1.f;
  if (a.x_amax != nullptr && a.x_amax_n < 0) {          // a cell-layout gradient: scaled when it was written
    xs_inv = reinterpret_cast<const float*>(a.x_amax)[1];
  } else if (a.x_amax != nullptr) {
    uint32_t* red = reinterpret_cast<uint32_t*>(ss + 2 * 64 * CT);
    uint32_t b = 0;
    for (int i = tid; i < a.x_amax_n; i += NT) b = a.x_amax[i] > b ? a.x_amax[i] : b;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)b, off, 64);
      b = o > b ? o : b;
    }
    if (lane == 0) red[wave] = b;
    __syncthreads();
    b = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) b = red[w] > b ? red[w] : b;
    const int e = (int)((b >> 23) & 0xFF);
    if (e != 0 && e != 255) {
      int sh = 127 + 14 - e;
      sh = sh > 100 ? 100 : (sh < -100 ? -100 : sh);
      xs = __builtin_bit_cast(float, (uint32_t)(127 + sh) << 23);
      xs_inv = __builtin_bit_cast(float, (uint32_t)(127 - sh) << 23);
    }
  }

  f32x16 accm[2][2], accl[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int i = 0; i < 16; ++i) { accm[r][m][i] = 0.f; accl[r][m][i] = 0.f; }

  // register sets: weights of stage s live in wv[s & 1]; patch slice g (= 3 * chunk + round) in pv[g & 1]
  u32x4 wv[2][WIT];
  float pv[2][8];
  auto load_w = [&](int stage, int set) {
    if constexpr (PAIR) {       // (the prologue's stages 0 and 1 of chunk pair 0; the stage loop passes its runs to load_runs)
#pragma unroll
      for (int k = 0; k < 2; ++k) wv[set][k] = wsrc[hs_pair_run(0, stage, k) + tid];
      return;
    }
    const u32x4* ws = wsrc + (size_t)stage * 768;
#pragma unroll
    for (int k = 0; k < WIT; ++k) wv[set][k] = ws[wsrc_off[k]];
  };
  auto store_w = [&](int set, int buf) {
#pragma unroll
    for (int k = 0; k < WIT; ++k) {
      u32x4* d = (WST % NT == 0 || wdst[k] >= 0) ? wl + buf * WST + wdst[k] : dummy + 2;
      *d = wv[set][k];
    }
  };
  auto load_p = [&](int chunk, int k, int set) {
    const uint32_t cbase = (uint32_t)chunk * kHsCC * plane_bytes;
    if (XCELLS) {           // the hi cell and, one plane (H W cells) further, the lo cell
      const u32x4 h4 = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, goff[k], cbase, 0);
      const u32x4 l4 = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, goff[k], cbase + 4 * plane_bytes, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pv[set][j] = u2f(h4[j]);
        pv[set][4 + j] = u2f(l4[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        pv[set][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, goff[k], cbase + j * plane_bytes, 0));
    }
  };
  auto store_p = [&](int set, int k, int buf) {
    u32x4 hi, lo;
    if (XCELLS) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        hi[j] = __builtin_bit_cast(uint32_t, pv[set][j]);
        lo[j] = __builtin_bit_cast(uint32_t, pv[set][4 + j]);
      }
    } else {
      split8(pv[set], xs, hi, lo);
    }
    u32x4* pd = patch + buf * COPY + pcell[k];
    u32x4* d0 = pcell[k] >= 0 ? pd : dummy;
    u32x4* d1 = pcell[k] >= 0 ? pd + PLANE : dummy + 1;
    *d0 = hi;
    *d1 = lo;
  };

  // 4 channels of a cell pair: hi + lo / 2^11, one v_fma_mix_f32 per value (fp16 operands converted inside the instruction; the
  // product with a power of two is exact, so this is the same value as convert, multiply, add -- in a third of the instructions)
  auto half4 = [](uint32_t h0, uint32_t h1, uint32_t l0, uint32_t l1, float* out) {
    const float inv = 1.f / kLoScale;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "=v"(out[0]) : "v"(l0), "s"(inv), "v"(h0));
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,1] op_sel_hi:[1,0,1]" : "=v"(out[1]) : "v"(l0), "s"(inv), "v"(h0));
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "=v"(out[2]) : "v"(l1), "s"(inv), "v"(h1));
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,1] op_sel_hi:[1,0,1]" : "=v"(out[3]) : "v"(l1), "s"(inv), "v"(h1));
  };

  const int pb_lane = khalf * KHP + (rowpair * 2) * PW + l31;
  const int wa_lane = slab * 768 + khalf * 64 + l31;

  // prologue: stage 0 complete in LDS; weights of stage 1 and the first slice of chunk 1 in flight
  load_w(0, 0);
  store_w(0, 0);
#pragma unroll
  for (int k = 0; k < PIT; ++k) { load_p(0, k, 0); store_p(0, k, 0); }
  load_w(1, 1);                 // nchunks is even (>= 2): stage 1 and chunk 1 exist
  if (tid < 2 * 64 * CT) ss[tid] = ssv;
  if (STATS == 2 && tid < 4 * 64 * CT) bsl[tid] = bsv;
  load_p(1, 0, 1);
  HS_TRACE(1);
  __syncthreads();
  HS_TRACE(2);

  if constexpr (PAIR) {
    const int j = lane & 15, kq = lane >> 4, ts = kq >> 1, kh2 = kq & 1;     // tap slot and k-half of the lane's k-group
    const int npairs = nchunks >> 1;
    f32x4 am[4][4], al[4][4];            // [channel block][pixel block]: hi*hi sums, cross-term sums (scaled by 2^11)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int pb = 0; pb < 4; ++pb)
#pragma unroll
        for (int i = 0; i < 4; ++i) { am[cb][pb][i] = 0.f; al[cb][pb][i] = 0.f; }
    // the lane's patch cell at column j of the wave's first row, per group of three stages (one pair of kernel rows and copies)
    const u32x4* pb_g[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      const HsPairTap t0 = hs_pair_stage(3 * g).tap[0], t1 = hs_pair_stage(3 * g).tap[1];
      pb_g[g] = patch + kh2 * KHP + (rowpair * 2) * PW + j + (ts ? t1.odd * COPY + t1.kh * PW : t0.odd * COPY + t0.kh * PW);
    }
    const int wa_pair = ts * 256 + kh2 * 64 + j;
    auto load_runs = [&](int o0, int o1, int set) {
      wv[set][0] = wsrc[o0 + tid];
      wv[set][1] = wsrc[o1 + tid];
    };
    // The nine stages of chunk pair `pair`; par = parity of the pair's first global stage (nine is odd: the register sets and the
    // weight buffers of a stage alternate with the GLOBAL stage, so the body exists once per parity and every index is a constant).
    // As in the 32x32x16 loop: weights two stages ahead into the set consumed last stage, a patch round one stage ahead of its
    // write; past the end the last stage / chunk is fetched again into buffers nobody reads.
    auto pair_stages = [&](const int par, const int pair) __attribute__((always_inline)) {
      const bool more = pair + 1 < npairs;
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        const int gp = (i + par) & 1;
        const HsPairStage st = hs_pair_stage(i), nx = hs_pair_stage((i + 1) % 9);
        if (i + 2 < 9) load_runs(hs_pair_run(pair, i + 2, 0), hs_pair_run(pair, i + 2, 1), gp);
        else load_runs(more ? hs_pair_run(pair + 1, i + 2 - 9, 0) : hs_pair_run(pair, 8, 0), more ? hs_pair_run(pair + 1, i + 2 - 9, 1) : hs_pair_run(pair, 8, 1), gp);
        if (nx.pround >= 0) {        // the round stage i + 1 writes: of this pair's o, the next pair's e or (i == 8) the next pair's o
          const int c = 2 * pair + 1 + (i == 8 ? 2 : nx.pnext);
          load_p(c < nchunks ? c : nchunks - 1, nx.pround, gp);
        }
        __builtin_amdgcn_sched_barrier(0);      // the fetches stay at the top of the stage
        const u32x4* pb0 = pb_g[i / 3] + i % 3;
        const u32x4* wa0 = wl + gp * WST + wa_pair;
        f16x8 A[2][4], B[2][4];
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
          for (int cb = 0; cb < 4; ++cb) A[pl][cb] = __builtin_bit_cast(f16x8, wa0[pl * 128 + cb * 16]);
#pragma unroll
          for (int pb = 0; pb < (XCELLS ? 4 : 2); ++pb) B[pl][pb] = __builtin_bit_cast(f16x8, pb0[pl * PLANE + (pb >> 1) * PW + (pb & 1) * 16]);
        }
#pragma unroll
        for (int pb = 0; pb < 4; ++pb) {
          if (!XCELLS && pb == 1) {
            // an fp32 input keeps eight staged values and the split's temporaries beside the accumulators: the second row's
            // fragments are read once the first pixel block's are dead
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int pl = 0; pl < 2; ++pl)
#pragma unroll
              for (int q = 2; q < 4; ++q) B[pl][q] = __builtin_bit_cast(f16x8, pb0[pl * PLANE + (q >> 1) * PW + (q & 1) * 16]);
          }
#pragma unroll
          for (int cb = 0; cb < 4; ++cb) {
            am[cb][pb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[0][cb], B[0][pb], am[cb][pb], 0, 0, 0);
            al[cb][pb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[0][cb], B[1][pb], al[cb][pb], 0, 0, 0);
          }
#pragma unroll
          for (int cb = 0; cb < 4; ++cb) al[cb][pb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[1][cb], B[0][pb], al[cb][pb], 0, 0, 0);
          if (pb == (XCELLS ? 0 : 1)) {
            // what arrived during the previous stage goes to LDS under this stage's remaining MFMAs (an fp32 input is split on
            // the way: behind the second pixel block, whose fragment registers the split's temporaries then take)
            store_w(gp ^ 1, gp ^ 1);
            if (st.pround >= 0) store_p(gp ^ 1, st.pround, st.pnext ? 0 : 1);
          }
        }
        __syncthreads();
      }
    };
    int pair = 0;
    for (; pair + 1 < npairs; pair += 2) {
      pair_stages(0, pair);
      pair_stages(1, pair + 1);
    }
    if (pair < npairs) pair_stages(0, pair);

    // ---- epilogue.  Accumulator lane (j, kq) holds channels 16 cb + 4 kq + i of pixel (row pb >> 1, column 16 (pb & 1) + j); the
    // v_permlane16_swap of a row's two pixel blocks leaves lane (j, kq) with channels 16 cb + 8 (kq >> 1) .. + 7 -- one cell -- of
    // the pixel at column ecol = 16 (kq & 1) + j: a half wave is 32 consecutive pixels of a channel plane (fp32 output: 128-byte
    // runs) or 32 consecutive cells.  Affine, residual (fp32, or cells through half4), ReLU and the range status as in MODE 0.
    const int ox = VROW ? xl : ox0 + ecol;
    const uint32_t plane_ob = (uint32_t)(a.OH * a.OW) * (uint32_t)sizeof(float);
    const uint32_t cplane = (uint32_t)(a.OH * a.OW) * 16u;
    const size_t img = (size_t)n * a.Cout * a.OH * a.OW;
    const int img_bytes = (int)(uint32_t)((VROW ? (uint32_t)a.N : 1u) * (uint32_t)a.Cout * plane_ob);
    const uint32_t img_off = VROW ? (uint32_t)nl * (uint32_t)a.Cout * plane_ob : 0u;
    const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(a.y + img, 0, img_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.res != nullptr ? a.res + img : a.y), 0, a.res != nullptr ? img_bytes : 0, 0x00020000);
    const uint32_t cbase_o = (uint32_t)cout0 * plane_ob;
    const uint32_t cell0 = (uint32_t)(cout0 >> 3) * 2u * cplane;
    const bool rcells = YCELLS && a.res_cells;
    bool inside[2];
    uint32_t vout[2], vres[2];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const int oy = oy0 + rowpair * 2 + rr;
      inside[rr] = lane_valid && oy < a.OH && ox < a.OW;
      const uint32_t pix = (uint32_t)(oy * a.OW + ox);
      const uint32_t vc = img_off + pix * 16u + (uint32_t)ts * 2u * cplane, vf = img_off + pix * 4u + (uint32_t)(8 * ts) * plane_ob;
      vout[rr] = !inside[rr] ? kOutside : (YCELLS ? vc : vf);
      vres[rr] = !inside[rr] ? kOutside : (rcells ? vc : vf);
    }
    float amax = 0.f;
    // The rest exists twice, with and without the residual path, as straight-line code behind ONE wave-uniform branch: a launch
    // without a residual (every conv1 of layer1) used to fetch it through an empty descriptor -- 64 buffer_load_dword per lane
    // that return zero -- which cost 5 us of the layer's 200 us launch (profiles/README.md, "Cell convs").  Such a launch keeps
    // the ADD of the zero: x + (+0) is +0 for x = -0, so the output stays what it was bit for bit.
    auto finish = [&](auto res_c) __attribute__((always_inline)) {
      constexpr bool RES = decltype(res_c)::value;
      uint32_t rraw[4][2][8];         // residual of the lane's cell (cb, rr): 8 floats, or the hi and lo cells as they are
      if constexpr (RES) {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
          for (int rr = 0; rr < 2; ++rr) {
            if (rcells) {
              const uint32_t so = cell0 + (uint32_t)(2 * cb) * 2u * cplane;
              const u32x4 h4 = __builtin_amdgcn_raw_buffer_load_b128(rrsrc, vres[rr], so, 0);
              const u32x4 l4 = __builtin_amdgcn_raw_buffer_load_b128(rrsrc, vres[rr], so + cplane, 0);
#pragma unroll
              for (int c = 0; c < 4; ++c) { rraw[cb][rr][c] = h4[c]; rraw[cb][rr][4 + c] = l4[c]; }
            } else {
#pragma unroll
              for (int c = 0; c < 8; ++c)
                rraw[cb][rr][c] = __builtin_amdgcn_raw_buffer_load_b32(rrsrc, vres[rr], cbase_o + (uint32_t)(16 * cb + c) * plane_ob, 0);
            }
          }
      }
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
          float o[8], r8[8];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int cl = 16 * cb + 4 * kq + i;
            float x = (am[cb][2 * rr][i] + al[cb][2 * rr][i] * (1.f / kLoScale)) * xs_inv;
            float y = (am[cb][2 * rr + 1][i] + al[cb][2 * rr + 1][i] * (1.f / kLoScale)) * xs_inv;
            x = x * ss[cl] + ss[64 + cl];
            y = y * ss[cl] + ss[64 + cl];
            const auto sw = __builtin_amdgcn_permlane16_swap(f2u(x), f2u(y), false, false);
            o[i] = u2f(sw[0]);
            o[4 + i] = u2f(sw[1]);
          }
          if constexpr (!RES) {
#pragma unroll
            for (int c = 0; c < 8; ++c) r8[c] = 0.f;
          } else if (rcells) {
            half4(rraw[cb][rr][0], rraw[cb][rr][1], rraw[cb][rr][4], rraw[cb][rr][5], r8);
            half4(rraw[cb][rr][2], rraw[cb][rr][3], rraw[cb][rr][6], rraw[cb][rr][7], r8 + 4);
          } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) r8[c] = u2f(rraw[cb][rr][c]);
          }
          float lm = 0.f;
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            const float t = o[c] + r8[c];
            o[c] = a.relu ? __builtin_fmaxf(t, 0.f) : t;
            lm = fp16_amax(lm, o[c]);
          }
          amax = fp16_amax(amax, inside[rr] ? lm : 0.f);
          if constexpr (YCELLS) {
            u32x4 hi, lo;
            split8(o, 1.f, hi, lo);
            const uint32_t so = cell0 + (uint32_t)(2 * cb) * 2u * cplane;
            __builtin_amdgcn_raw_buffer_store_b128(hi, yrsrc, vout[rr], so, 0);
            __builtin_amdgcn_raw_buffer_store_b128(lo, yrsrc, vout[rr], so + cplane, 0);
            asm volatile("s_nop 0" ::"v"(hi), "v"(lo));      // (cells_store32: a VALU write in the store's next issue slot)
          } else {
#pragma unroll
            for (int c = 0; c < 8; ++c)
              __builtin_amdgcn_raw_buffer_store_b32(f2u(o[c]), yrsrc, vout[rr], cbase_o + (uint32_t)(16 * cb + c) * plane_ob, 0);
          }
        }
    };
    // (the fp32-input forms -- single launches outside the executor, already over their register budget -- keep the one epilogue)
    if (!XCELLS || a.res != nullptr) finish(std::true_type{});
    else finish(std::false_type{});
    range_flag(a.status, out_of_fp16(amax));
    return;
  }

  for (int cp = 0; cp < nchunks; cp += 2) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int s = 3 * cp + i;                 // global stage; s & 1 == i & 1 because cp is even
      const int kh = i % 3, cpar = (i / 3) & 1; // kernel row, parity of this stage's chunk
      const u32x4* pb0 = patch + cpar * COPY + pb_lane;
      const u32x4* wa0 = wl + (i & 1) * WST + wa_lane;
      // fetch two stages ahead (weights of s+2, patch slice s+4) into the sets that were consumed last stage
      // (past the end the last stage / chunk is fetched again and its copy in the idle buffers is never read)
      load_w(s + 2 < nstages ? s + 2 : nstages - 1, i & 1);
      if ((i + 1) % 3 < PIT) load_p(s + 4 < nstages ? (s + 4) / 3 : nchunks - 1, (i + 1) % 3, i & 1);
      __builtin_amdgcn_sched_barrier(0);      // the fetches stay at the top of the stage: two stages of latency cover
#pragma unroll
      for (int kw = 0; kw < K; ++kw) {
        f16x8 A[2][2], B[2][2];
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
          for (int m = 0; m < 2; ++m) A[pl][m] = __builtin_bit_cast(f16x8, wa0[(kw * 2 + pl) * 128 + m * 32]);
#pragma unroll
          for (int r = 0; r < 2; ++r) B[pl][r] = __builtin_bit_cast(f16x8, pb0[pl * PLANE + (r + kh) * PW + kw]);
        }
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int m = 0; m < 2; ++m) {
            accm[r][m] = hs_mfma(A[0][m], B[0][r], accm[r][m]);
            accl[r][m] = hs_mfma(A[0][m], B[1][r], accl[r][m]);
            accl[r][m] = hs_mfma(A[1][m], B[0][r], accl[r][m]);
          }
        if (kw == 0) {
          // what arrived during the previous stage goes to LDS under this stage's remaining MFMAs:
          // weights of stage s+1 -> the other weight buffer, patch slice s+3 -> the next chunk's patch copy
          store_w((i + 1) & 1, (i + 1) & 1);
          if (i % 3 < PIT) store_p((i + 1) & 1, i % 3, ((i + 3) / 3) & 1);
        }
      }
      __syncthreads();
    }
  }

  HS_TRACE(3);
  // epilogue through buffer descriptors: one instruction per access (wave-uniform channel offset in an SGPR, the
  // lane's pixel in one 32-bit VGPR); lanes outside the map carry the out-of-range offset, so their loads return 0
  // and their stores are dropped; without a residual the descriptor is empty and every load returns 0
  const int ox = VROW ? xl : ox0 + ecol;
  const uint32_t plane_ob = (uint32_t)(a.OH * a.OW) * (uint32_t)sizeof(float);
  const size_t img = (size_t)n * a.Cout * a.OH * a.OW;
  // YCELLS: the descriptors cover the whole tensors and the lane's image rides in its offset
  const int img_bytes = (int)(uint32_t)((VROW ? (uint32_t)a.N : 1u) * (uint32_t)a.Cout * plane_ob);
  const uint32_t img_off = VROW ? (uint32_t)nl * (uint32_t)a.Cout * plane_ob : 0u;
  float* const ybase = a.ksplit > 1 ? a.part + (size_t)kpart * a.part_stride : a.y;
  const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(ybase + img, 0, img_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rrsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.res != nullptr ? a.res + img : a.y), 0, a.res != nullptr ? img_bytes : 0, 0x00020000);
  const float* sst = ss + slab * 64;
  const uint32_t cbase_o = (uint32_t)cout0 * plane_ob;
  const uint32_t cplane = (uint32_t)(a.OH * a.OW) * 16u;                  // one plane of cells of the output map, bytes
  const uint32_t cell0 = (uint32_t)(cout0 >> 3) * 2u * cplane;            // first cell (hi plane) of this wave's 64 channels
  bool inside[2];
  uint32_t pix[2];
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    const int oy = oy0 + rowpair * 2 + rr;
    inside[rr] = lane_valid && oy < a.OH && ox < a.OW;
    pix[rr] = (uint32_t)(oy * a.OW + ox);
  }
  float amax = 0.f;        // range status (adx_common.h: fp16_amax); a.status is null for the partial sums of a split reduction
  if constexpr (YCELLS) {
    // cell output (cells_store32); the residual is fetched first: as cells, or as fp32 values at the channels the lane owns AFTER the swap
    const uint32_t khoff = (uint32_t)khalf * 2u * cplane;                  // this lane's cells are the odd ones: one cell further
    uint32_t vcell[2], vres[2];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      vcell[rr] = inside[rr] ? img_off + pix[rr] * 16u + khoff : kOutside;
      vres[rr] = !inside[rr] ? kOutside : a.res_cells ? vcell[rr] : img_off + pix[rr] * 4u + (uint32_t)(8 * khalf) * plane_ob;
    }
    uint32_t rraw[2][2][2][8];          // residual of cell (rr, half, i): 8 floats, or the hi and lo cells as they are
#pragma unroll
    for (int rr = 0; rr < 2; ++rr)
#pragma unroll
      for (int half = 0; half < 2; ++half)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          if (a.res_cells) {
            const uint32_t so = cell0 + (uint32_t)(half * 4 + 2 * i) * 2u * cplane;
            const u32x4 h4 = __builtin_amdgcn_raw_buffer_load_b128(rrsrc, vres[rr], so, 0);
            const u32x4 l4 = __builtin_amdgcn_raw_buffer_load_b128(rrsrc, vres[rr], so + cplane, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) { rraw[rr][half][i][j] = h4[j]; rraw[rr][half][i][4 + j] = l4[j]; }
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
              rraw[rr][half][i][j] = __builtin_amdgcn_raw_buffer_load_b32(rrsrc, vres[rr], cbase_o + (uint32_t)(half * 32 + 16 * i + j) * plane_ob, 0);
          }
        }
#ifdef ADX_HS_TRACE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    HS_TRACE(6);
#endif
#pragma unroll
    for (int rr = 0; rr < 2; ++rr)
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        float v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = accm[rr][half][r] + accl[rr][half][r] * (1.f / kLoScale);      // no dynamic range here: xs = 1
        float res8[2][8];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          if (a.res_cells) {
            half4(rraw[rr][half][i][0], rraw[rr][half][i][1], rraw[rr][half][i][4], rraw[rr][half][i][5], res8[i]);
            half4(rraw[rr][half][i][2], rraw[rr][half][i][3], rraw[rr][half][i][6], rraw[rr][half][i][7], res8[i] + 4);
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) res8[i][j] = u2f(rraw[rr][half][i][j]);
          }
        }
        cells_store32(v, sst, sst + 64 * CT, half * 32 + 8 * khalf, res8, a.relu != 0, yrsrc, vcell[rr],
                      cell0 + (uint32_t)(half * 4) * 2u * cplane, cplane, amax);
      }
  } else {
  uint32_t voff[2];
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) voff[rr] = inside[rr] ? img_off + pix[rr] * 4u + (uint32_t)(4 * khalf) * plane_ob : kOutside;
  float rv[2][2][16];
  if constexpr (STATS != 2) {
#pragma unroll
  for (int rr = 0; rr < 2; ++rr)
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cu = half * 32 + (r & 3) + 8 * (r >> 2);     // + 4 * khalf, which rides in voff
        rv[rr][half][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rrsrc, voff[rr], cbase_o + cu * plane_ob, 0));
      }
  }
#ifdef ADX_HS_TRACE
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  HS_TRACE(6);
#endif
  if constexpr (STATS != 0) {
    // Per-channel partial sums of this workgroup's pixels (those outside the map excluded), so that a BatchNorm needs no pass
    // over the tensor this launch writes.  STATS == 1 (training forward): sum and sum of squares of the conv output.  STATS
    // == 2 (data gradient): dx = conv + residual is finished and stored HERE, and the sums are those of the BatchNorm backward
    // of the layer dx flows into: sum dz and sum dz xhat, dz = dx where that layer's ReLU let the value through.
    // Per (half, r) register: the two rows of the lane, then the 16 lanes of a DPP row; lanes 0 / 16 / 32 / 48 park their row's
    // totals in LDS (the patch is dead: every wave passed the main loop's last barrier), 64 CT x 2 threads add the 2 x NW/CT
    // rows up in a fixed order.
    float* red = reinterpret_cast<float*>(smem_raw);          // [wave][lane >> 4][32][2]
    const bool val0 = voff[0] != kOutside, val1 = voff[1] != kOutside;
    auto park = [&](int half, int r, float sm, float sq) {
      sm += hs_dpp<0xB1>(sm);  sq += hs_dpp<0xB1>(sq);      // quad_perm [1,0,3,2]
      sm += hs_dpp<0x4E>(sm);  sq += hs_dpp<0x4E>(sq);      // quad_perm [2,3,0,1]
      sm += hs_dpp<0x141>(sm); sq += hs_dpp<0x141>(sq);     // row_half_mirror
      sm += hs_dpp<0x140>(sm); sq += hs_dpp<0x140>(sq);     // row_mirror: every lane of a row of 16 holds the row's total
      if ((lane & 15) == 0) {
        float* d = red + (((wave * 4 + (lane >> 4)) * 32) + half * 16 + r) * 2;
        d[0] = sm;
        d[1] = sq;
      }
    };
    if constexpr (STATS == 1) {
#pragma unroll
      for (int half = 0; half < 2; ++half)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float v0 = val0 ? (accm[0][half][r] + accl[0][half][r] * (1.f / kLoScale)) * xs_inv : 0.f;
          const float v1 = val1 ? (accm[1][half][r] + accl[1][half][r] * (1.f / kLoScale)) * xs_inv : 0.f;
          park(half, r, v0 + v1, v0 * v0 + v1 * v1);
        }
    } else {
      // the accumulators fold into accm first (accl is dead afterwards); then one 32-channel half at a time: residual, conv
      // output of the consumer BatchNorm (xhat, and its ReLU mask when the ReLU sits straight behind it) and, otherwise, that
      // layer's output (the mask) are fetched together -- 96 loads in flight -- and dx is stored from the same registers
#pragma unroll
      for (int rr = 0; rr < 2; ++rr)
#pragma unroll
        for (int half = 0; half < 2; ++half)
#pragma unroll
          for (int r = 0; r < 16; ++r) accm[rr][half][r] = (accm[rr][half][r] + accl[rr][half][r] * (1.f / kLoScale)) * xs_inv;
      const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.bs_raw + img), 0, img_bytes, 0x00020000);
      const bool mask_bits = a.bs_mask == 1 && a.bs_bits != nullptr;       // the forward's mask bits instead of its fp32 output
      const bool mask_out = a.bs_mask == 1 && !mask_bits;
      const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(mask_out ? a.bs_out + img : a.y), 0, mask_out ? img_bytes : 0, 0x00020000);
      // mask bits: byte [n][c / 8][pixel]; this lane's channels of a register group r >> 2 are bits 4 khalf .. 4 khalf + 3 of one byte
      const uint32_t bplane = (uint32_t)(a.OH * a.OW);
      const __amdgpu_buffer_rsrc_t brsrc = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<uint8_t*>(mask_bits ? a.bs_bits + (size_t)n * (a.Cout >> 3) * bplane : reinterpret_cast<const uint8_t*>(a.y)), 0,
          mask_bits ? (int)((VROW ? (uint32_t)a.N : 1u) * (uint32_t)(a.Cout >> 3) * bplane) : 0, 0x00020000);
      uint32_t boff[2];
#pragma unroll
      for (int rr = 0; rr < 2; ++rr)
        boff[rr] = inside[rr] ? (VROW ? (uint32_t)nl * (uint32_t)(a.Cout >> 3) * bplane : 0u) + pix[rr] : kOutside;
      // the residual's own mask bits (same layout): the identity path's gradient is res where the block's output was positive
      const bool res_masked = a.res_bits != nullptr;
      const __amdgpu_buffer_rsrc_t qrsrc = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<uint8_t*>(res_masked ? a.res_bits + (size_t)n * (a.Cout >> 3) * bplane : reinterpret_cast<const uint8_t*>(a.y)), 0,
          res_masked ? (int)((VROW ? (uint32_t)a.N : 1u) * (uint32_t)(a.Cout >> 3) * bplane) : 0, 0x00020000);
      const float* bsw = bsl + slab * 64;
      const uint32_t use_bit = mask_bits ? 1u : 0u, use_out = mask_out ? 1u : 0u, use_raw = 1u - use_bit - use_out;
      const uint32_t v0u = val0 ? 1u : 0u, v1u = val1 ? 1u : 0u;
      float dmx = 0.f;          // max |dz| of this lane: the BatchNorm-backward apply pass bounds its output's range with it
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        float rs_[2][16], rw_[2][16], ro_[2][16];
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const uint32_t so = cbase_o + (uint32_t)(half * 32 + (r & 3) + 8 * (r >> 2)) * plane_ob;
            rs_[rr][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rrsrc, voff[rr], so, 0));
            rw_[rr][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wrsrc, voff[rr], so, 0));
            ro_[rr][r] = 0.f;
          }
        if (mask_out) {        // wave-uniform: the 32 loads of the consumer layer's output only where its ReLU follows the residual add
#pragma unroll
          for (int rr = 0; rr < 2; ++rr)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const uint32_t so = cbase_o + (uint32_t)(half * 32 + (r & 3) + 8 * (r >> 2)) * plane_ob;
              ro_[rr][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(orsrc, voff[rr], so, 0));
            }
        }
        if (res_masked) {      // wave-uniform
#pragma unroll
          for (int rr = 0; rr < 2; ++rr)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const uint32_t m = (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(qrsrc, boff[rr], ((uint32_t)(cout0 >> 3) + (uint32_t)(half * 4 + q)) * bplane, 0)
                                 >> (4 * khalf);
#pragma unroll
              for (int i = 0; i < 4; ++i)
                if (!((m >> i) & 1u)) rs_[rr][4 * q + i] = 0.f;
            }
        }
        uint32_t mb[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
        if (mask_bits) {       // eight byte loads instead
#pragma unroll
          for (int rr = 0; rr < 2; ++rr)
#pragma unroll
            for (int q = 0; q < 4; ++q)
              mb[rr][q] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(brsrc, boff[rr], ((uint32_t)(cout0 >> 3) + (uint32_t)(half * 4 + q)) * bplane, 0)
                          >> (4 * khalf);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int cu = half * 32 + (r & 3) + 8 * (r >> 2);
          const int cl = cu + 4 * khalf;
          const float mu = bsw[cl], rsd = bsw[64 * CT + cl], msc = bsw[2 * 64 * CT + cl], msh = bsw[3 * 64 * CT + cl];
          float p[2], q[2];
#pragma unroll
          for (int rr = 0; rr < 2; ++rr) {
            const float y = accm[rr][half][r] + rs_[rr][r];            // scale 1, shift 0, no ReLU: what `finish` would store
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, y), yrsrc, voff[rr], cbase_o + cu * plane_ob, 0);
            // all three forms of the consumer's ReLU mask evaluated, one SELECTED (the choice is uniform over the launch), the
            // lane's validity folded in by `&`: as val && (bits ? .. : (out ? .. : ..)) it was four branches per value, 270 per tile
            // (as integer masks: a select between booleans on a uniform condition is turned back into a branch)
            const uint32_t on_bit = (mb[rr][r >> 2] >> (r & 3)) & 1u, on_out = ro_[rr][r] > 0.f ? 1u : 0u;
            const uint32_t on_raw = __builtin_fmaf(rw_[rr][r], msc, msh) > 0.f ? 1u : 0u;
            const bool keep = ((rr == 0 ? v0u : v1u) & ((on_bit & use_bit) | (on_out & use_out) | (on_raw & use_raw))) != 0u;
            p[rr] = keep ? y : 0.f;
            q[rr] = p[rr] * ((rw_[rr][r] - mu) * rsd);
            dmx = __builtin_fmaxf(dmx, __builtin_fabsf(p[rr]));
          }
          park(half, r, p[0] + p[1], q[0] + q[1]);
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) dmx = __builtin_fmaxf(dmx, __shfl_xor(dmx, off, 64));
      if (lane == 0) red[4096 + wave] = dmx;
    }
    __syncthreads();
    if (STATS == 2 && tid >= 2 * 64 * CT && tid < 2 * 64 * CT + CT) {      // one thread per 64-channel slab: max over its waves
      const int sl = tid - 2 * 64 * CT;
      constexpr int WPS = (NT / 64) / CT;
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < WPS; ++w) t = __builtin_fmaxf(t, red[4096 + (MODE == 2 ? sl * WPS + w : w)]);
      const int p = (n * a.tiles_y + ty) * a.tiles_x + tx;
      a.stats_part[(size_t)a.Cout * 2 * a.stats_p + (size_t)(ct * CT + sl) * a.stats_p + p] = t;
    }
    if (tid < 2 * 64 * CT) {
      const int which = tid & 1, chs = tid >> 1, sl = chs >> 6, ch = chs & 63;     // channel ch of slab sl
      const int c5 = ch & 31, kh2 = (c5 >> 2) & 1, r = (c5 & 3) + 4 * (c5 >> 3), idx32 = (ch >> 5) * 16 + r;
      constexpr int WPS = (NT / 64) / CT;                   // waves per slab
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < WPS; ++w)
#pragma unroll
        for (int j = 0; j < 2; ++j) t += red[((((MODE == 2 ? sl * WPS + w : w) * 4 + kh2 * 2 + j) * 32) + idx32) * 2 + which];
      const int p = (n * a.tiles_y + ty) * a.tiles_x + tx;
      a.stats_part[((size_t)((ct * CT + sl) * kHsCout + ch) * 2 + which) * a.stats_p + p] = t;
    }
  }
  auto finish = [&](auto relu) {       // two copies of the store loop: the ReLU is one v_max, not a compare + select
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      float lm = 0.f;       // this row's values; only a pixel of the map counts
#pragma unroll
      for (int half = 0; half < 2; ++half)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int cu = half * 32 + (r & 3) + 8 * (r >> 2);
          const int cl = cu + 4 * khalf;
          float v = (accm[rr][half][r] + accl[rr][half][r] * (1.f / kLoScale)) * xs_inv;
          v = v * sst[cl] + sst[64 * CT + cl];
          v += rv[rr][half][r];
          if (decltype(relu)::value) v = __builtin_fmaxf(v, 0.f);   // a NaN becomes 0, like `v > 0 ? v : 0` did
          lm = fp16_amax(lm, v);
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), yrsrc, voff[rr], cbase_o + cu * plane_ob, 0);
        }
      amax = fp16_amax(amax, inside[rr] ? lm : 0.f);
    }
  };
  if constexpr (STATS != 2) {
    if (a.relu) finish(std::true_type{}); else finish(std::false_type{});
  }
  }
  range_flag(a.status, out_of_fp16(amax));
  HS_TRACE(4);
#ifdef ADX_HS_TRACE
  __builtin_amdgcn_s_waitcnt(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  HS_TRACE(5);
#endif
}

// ---- the stem: Conv2d(3, 64, 7, stride 2, padding 3), modeling/resnet.py:191 --------------------------------
// K = 3 channels x 7 x 7 = 147 has no 16-channel chunks, so the GEMM's k axis is laid out as 21 (channel, kernel
// row) "combos" x 8 kernel columns (7 real + one zero weight): a lane's B fragment -- 8 consecutive k for one
// output pixel -- is then 8 CONSECUTIVE input columns of one patch row, i.e. 16 contiguous bytes of the fp16 patch
// image [plane][channel][row][column] (read as 4 dwords: the start column 2*ox is only 4-byte aligned), and one
// MFMA (K = 16) covers two combos.  11 k-steps x 3 products per 32x32 tile; 84 % of the k slots are real work.
// Both stem kernels below share this layout, the weight image (conv2d_hs_stem_pack_kernel) and the k-step order, so
// a stem value is bit for bit the same whichever of them computes it.
constexpr int kStemSteps = 11;
constexpr int kStemPP = 72;                               // patch row pitch in halves (70 columns are staged)
constexpr int kStemPH = 21;                               // patch rows of a band of 8 stem rows

// One 32x32x(64 channels) stem tile of one stem row (patch row prow of the staged band), accumulated in the k-step order
// that both stem kernels share: the fragments of step s+1 are read under the MFMAs of step s.
struct StemFrags { f16x8 A[2][2], B[2]; };
__device__ __forceinline__ void stem_tile(const u32x4* wa0, const uint32_t* pb0, int khalf, f32x16 (&accm)[2], f32x16 (&accl)[2]) {
  constexpr int CP = kStemPH * kStemPP, PLANEH = 3 * CP;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int i = 0; i < 16; ++i) { accm[m][i] = 0.f; accl[m][i] = 0.f; }
  auto fetch = [&](StemFrags& f, int step) {
    // this lane's (channel, kernel row): combo 2*step + khalf; the 22nd combo has zero weights, re-reads the 21st
    const int c0 = 2 * step, c1 = 2 * step + 1 > 20 ? 20 : 2 * step + 1;
    const int off0 = ((c0 / 7) * CP + (c0 % 7) * kStemPP) / 2, off1 = ((c1 / 7) * CP + (c1 % 7) * kStemPP) / 2;
    const uint32_t* pb = pb0 + (khalf ? off1 : off0);
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
      for (int m = 0; m < 2; ++m) f.A[pl][m] = __builtin_bit_cast(f16x8, wa0[(step * 2 + pl) * 128 + m * 32]);
      const uint32_t* q = pb + pl * (PLANEH / 2);
      u32x4 v;
      v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
      f.B[pl] = __builtin_bit_cast(f16x8, v);
    }
  };
  StemFrags fr[2];
  fetch(fr[0], 0);
#pragma unroll
  for (int step = 0; step < kStemSteps; ++step) {
    if (step + 1 < kStemSteps) fetch(fr[(step + 1) & 1], step + 1);
    __builtin_amdgcn_sched_barrier(0);
    const StemFrags& f = fr[step & 1];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      accm[m] = hs_mfma(f.A[0][m], f.B[0], accm[m]);
      accl[m] = hs_mfma(f.A[0][m], f.B[1], accl[m]);
      accl[m] = hs_mfma(f.A[1][m], f.B[0], accl[m]);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// The band's patch: 3 channels x kStemPH rows x 35 column pairs, split into [plane][channel][row][pitch] halves.  Thread t < 245
// owns column pair t % 35 of the rows (channel, row) = t / 35 + 7 k, k < 9: its geometry costs one division per thread, not one
// per cell, and a cell's (channel, row) is two compares off its k (no chain of dependent address updates).
constexpr int kStemStageItems = 3 * kStemPH / 7;
template <bool U8>
struct StemStager {
  float pv[kStemStageItems][2];
  float amax = 0.f;     // max |x| over the input values store() splits (adx_common.h: fp16_amax); outside the frame they are 0
  __device__ __forceinline__ void load(const Conv2dArgs& a, __amdgpu_buffer_rsrc_t xrsrc, int r0, int ix, int iy0) {
    constexpr uint32_t kOutside = 0xC0000000u;
    const bool act = r0 < 7;
    const bool ok0 = act && ix >= 0 && ix < a.W, ok1 = act && ix + 1 >= 0 && ix + 1 < a.W;
    const size_t hw = (size_t)a.H * a.W;
#pragma unroll
    for (int k = 0; k < kStemStageItems; ++k) {
      const int rc = r0 + 7 * k;
      const int c = (rc >= kStemPH) + (rc >= 2 * kStemPH), iy = iy0 + rc - kStemPH * c;
      const bool rok = iy >= 0 && iy < a.H;
      const bool v0 = rok && ok0, v1 = rok && ok1;
      if (U8) {
        // uint8 HWC frame: byte (iy, ix, c); outside the frame the NORMALISED tensor is zero-padded, so the value is 0
        // there, not normalise(0).  Same operation order as image_normalize_kernel (IEEE division, no contraction).
#pragma clang fp contract(off)
        const uint32_t brow = (uint32_t)(iy * a.W) * 3u + (uint32_t)c;
        const uint32_t b0 = __builtin_amdgcn_raw_buffer_load_b8(xrsrc, v0 ? brow + (uint32_t)ix * 3u : kOutside, 0, 0);
        const uint32_t b1 = __builtin_amdgcn_raw_buffer_load_b8(xrsrc, v1 ? brow + (uint32_t)(ix + 1) * 3u : kOutside, 0, 0);
        const float mean = c == 0 ? a.u8_mean[0] : (c == 1 ? a.u8_mean[1] : a.u8_mean[2]);
        const float stdv = c == 0 ? a.u8_std[0] : (c == 1 ? a.u8_std[1] : a.u8_std[2]);
        pv[k][0] = v0 ? ((float)b0 / 255.0f - mean) / stdv : 0.f;
        pv[k][1] = v1 ? ((float)b1 / 255.0f - mean) / stdv : 0.f;
      } else {
        const uint32_t grow = (uint32_t)(c * (int)hw + iy * a.W) * 4u;
        pv[k][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, v0 ? grow + (uint32_t)ix * 4u : kOutside, 0, 0));
        pv[k][1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, v1 ? grow + (uint32_t)(ix + 1) * 4u : kOutside, 0, 0));
      }
    }
  }
  __device__ __forceinline__ void store(uint32_t* pd, int r0, int pp) {
    constexpr int PLANEH = 3 * kStemPH * kStemPP;
    if (r0 >= 7) return;
#pragma unroll
    for (int k = 0; k < kStemStageItems; ++k) {
      f16x2 h, l;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const _Float16 hj = (_Float16)pv[k][j];
        amax = fp16_amax(amax, pv[k][j]);
        h[j] = hj;
        l[j] = (_Float16)((pv[k][j] - (float)hj) * kLoScale);
      }
      // (channel, row) r0 + 7 k is row r0 + 7 k of the [channel][row] stack: the pitch is uniform across channels
      const int dw = ((r0 + 7 * k) * kStemPP) / 2 + pp;
      pd[dw] = __builtin_bit_cast(uint32_t, h);
      pd[PLANEH / 2 + dw] = __builtin_bit_cast(uint32_t, l);
    }
  }
};

// The plain stem (training forward, ops.conv2d at k = 7): one workgroup owns a band of 8 output rows of one image and walks
// its 32-column tiles; wave w computes rows 2 w, 2 w + 1.  The 45 KB split weight image is loaded into LDS once per band,
// the patch of tile i+1 is fetched while tile i is multiplied (two patch copies).
__global__ void __launch_bounds__(256, 2) conv2d_hs_stem_kernel(const Conv2dArgs a) {
  constexpr int CP = kStemPH * kStemPP;                    // halves per channel plane
  constexpr int PLANEH = 3 * CP;                           // halves per split plane
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  u32x4* wl = reinterpret_cast<u32x4*>(smem_raw);                         // [step][plane][k-half][64]
  uint32_t* patch = reinterpret_cast<uint32_t*>(wl + kStemSteps * 256);   // 2 x [plane][channel][row][pitch/2] dwords
  float* ss = reinterpret_cast<float*>(patch + 2 * PLANEH);               // a buffer = 2 planes x PLANEH/2 dwords
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, khalf = lane >> 5;
  int bid = blockIdx.x, seg = 0;
  if (a.stem_nseg > 1) { seg = bid % a.stem_nseg; bid /= a.stem_nseg; }
  const int n = bid / a.tiles_y, ty = bid - n * a.tiles_y;
  const int tx_begin = a.stem_nseg > 1 ? seg * a.stem_seg_tiles : 0;
  const int tx_end = a.stem_nseg > 1 ? min(a.tiles_x, tx_begin + a.stem_seg_tiles) : a.tiles_x;
  const int oy0 = ty * 8, iy0 = oy0 * 2 - 3;               // first stem row of the band
  const size_t hw = (size_t)a.H * a.W;
  const __amdgpu_buffer_rsrc_t xrsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x + (size_t)n * 3 * hw), 0, (int)(3 * hw * sizeof(float)), 0x00020000);

  {
    const u32x4* wsrc = reinterpret_cast<const u32x4*>(a.w);
#pragma unroll
    for (int k = 0; k < kStemSteps; ++k) wl[tid + 256 * k] = wsrc[tid + 256 * k];
  }
  if (tid < 2 * kHsCout) {
    const int c = tid & (kHsCout - 1);
    ss[tid] = a.scale == nullptr ? (tid < kHsCout ? 1.f : 0.f) : (tid < kHsCout ? a.scale[c] : a.shift[c]);
  }
  const int r0 = tid / 35, pp = tid - r0 * 35;              // staging geometry (StemStager)
  StemStager<false> sg;
  const u32x4* wa0 = wl + khalf * 64 + l31;
  const size_t img = (size_t)n * a.Cout * a.OH * a.OW;
  // stores through a buffer descriptor: channel offset in an SGPR, the lane's pixel in one VGPR (out of range = dropped)
  const uint32_t plane_ob = (uint32_t)(a.OH * a.OW) * (uint32_t)sizeof(float);
  const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(a.y + img, 0, (int)(a.Cout * plane_ob), 0x00020000);
  constexpr uint32_t kOutside = 0xC0000000u;

  sg.load(a, xrsrc, r0, tx_begin * 64 - 3 + 2 * pp, iy0);
  sg.store(patch + (tx_begin & 1) * PLANEH, r0, pp);
  __syncthreads();
  for (int tx = tx_begin; tx < tx_end; ++tx) {
    if (tx + 1 < tx_end) sg.load(a, xrsrc, r0, (tx + 1) * 64 - 3 + 2 * pp, iy0);
    const int ox = tx * kTileW + l31;
    // both rows of the wave in one pass: the A fragments of a k-step serve four products each
    const uint32_t* pb0 = patch + (tx & 1) * PLANEH + wave * 4 * (kStemPP / 2) + l31;
    f32x16 accm[2][2], accl[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int i = 0; i < 16; ++i) { accm[r][m][i] = 0.f; accl[r][m][i] = 0.f; }
#pragma unroll 1
    for (int step = 0; step < kStemSteps; ++step) {
      const int c0 = 2 * step, c1 = 2 * step + 1 > 20 ? 20 : 2 * step + 1;     // as stem_tile
      const int off0 = ((c0 / 7) * CP + (c0 % 7) * kStemPP) / 2, off1 = ((c1 / 7) * CP + (c1 % 7) * kStemPP) / 2;
      const uint32_t* pb = pb0 + (khalf ? off1 : off0);
      f16x8 A[2][2], B[2][2];
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
        for (int m = 0; m < 2; ++m) A[pl][m] = __builtin_bit_cast(f16x8, wa0[(step * 2 + pl) * 128 + m * 32]);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const uint32_t* q = pb + pl * (PLANEH / 2) + r * 2 * (kStemPP / 2);
          u32x4 v;
          v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
          B[pl][r] = __builtin_bit_cast(f16x8, v);
        }
      }
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          accm[r][m] = hs_mfma(A[0][m], B[0][r], accm[r][m]);
          accl[r][m] = hs_mfma(A[0][m], B[1][r], accl[r][m]);
          accl[r][m] = hs_mfma(A[1][m], B[0][r], accl[r][m]);
        }
    }
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const int oy = oy0 + wave * 2 + rr;
      const uint32_t voff = (oy < a.OH && ox < a.OW) ? (uint32_t)(oy * a.OW + ox) * 4u + (uint32_t)(4 * khalf) * plane_ob : kOutside;
#pragma unroll
      for (int half = 0; half < 2; ++half)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int cu = half * 32 + (r & 3) + 8 * (r >> 2);
          const int cl = cu + 4 * khalf;
          float v = accm[rr][half][r] + accl[rr][half][r] * (1.f / kLoScale);
          v = v * ss[cl] + ss[kHsCout + cl];
          if (a.relu) v = v > 0.f ? v : 0.f;
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), yrsrc, voff, cu * plane_ob, 0);
        }
    }
    if (tx + 1 < tx_end) sg.store(patch + ((tx + 1) & 1) * PLANEH, r0, pp);
    __syncthreads();
  }
}

// The stem + BN + ReLU + MaxPool2d(3, 2, 1) (modeling/resnet.py:197) in one launch: only the pooled map is written, the
// stem's own output (944 MB at B = 64, 3x256x900 -- the largest tensor of the network) is never stored nor re-read.
// Every stem row is computed ONCE.  A workgroup owns a strip of 32 stem columns of one image and walks it down in bands
// of 8 stem rows = 4 pooled rows; wave w computes stem rows 2p and 2p + 1 of pooled row p = 4 band + w.
//  * horizontally a strip's columns are 30 tx - 1 .. 30 tx + 30 (neighbouring strips overlap by two columns): pooled
//    column 15 tx + i is the maximum over lanes 2i, 2i + 1, 2i + 2 of one 32-lane group, taken with two DPP shifts before
//    anything leaves the registers.  450 stem columns are 15 strips of 30, as many MFMA columns as 32-column tiles had;
//  * vertically pooled row p also needs stem row 2p - 1: the odd row of wave w - 1, or for wave 0 the odd row of the
//    previous band's wave 3.  Each wave parks its odd row's horizontal maxima (15 columns x 64 channels) in LDS; after
//    one barrier wave w >= 1 folds in wave w - 1's, and wave 0 takes wave 3's as the start of its next row.  A walk that
//    does not start at the top (few images: the strip is cut into segments) first computes only the odd rows of the band
//    in front of it.
// Every value that reaches a maximum is >= 0 or the padding's -inf (the ReLU maps a NaN stem value to 0, as `v > 0 ? v : 0`
// does), so the maxima are plain v_max / v_max3: torch's rule that a NaN in the window wins has nothing to decide.
// One patch copy: the next band is fetched into registers under the MFMAs and split into LDS behind the exchange barrier,
// so the walk costs two barriers per band.  45 KB weights + 18 KB patch + 16 KB exchange: two workgroups per CU.
constexpr int kStemPoolCols = 15;            // pooled columns per strip
template <bool U8>
__global__ void __launch_bounds__(256, 2) conv2d_hs_stem_pool_kernel(const Conv2dArgs a) {
  constexpr int PLANEH = 3 * kStemPH * kStemPP;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  u32x4* wl = reinterpret_cast<u32x4*>(smem_raw);                         // [step][plane][k-half][64]
  uint32_t* patch = reinterpret_cast<uint32_t*>(wl + kStemSteps * 256);   // [plane][channel][row][pitch/2] dwords
  float* ss = reinterpret_cast<float*>(patch + PLANEH);
  float* xch = ss + 2 * kHsCout;                                          // [wave][32 registers][k-half][16 pooled columns]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, khalf = lane >> 5;
  int bid = blockIdx.x, seg = 0;
  if (a.stem_nseg > 1) { seg = bid % a.stem_nseg; bid /= a.stem_nseg; }
  const int n = bid / a.tiles_x, tx = bid - n * a.tiles_x;
  const int b_own = a.stem_nseg > 1 ? seg * a.stem_seg_tiles : 0;
  const int b_end = a.stem_nseg > 1 ? min(a.tiles_y, b_own + a.stem_seg_tiles) : a.tiles_y;
  const int b_begin = b_own > 0 ? b_own - 1 : 0;
  const int sx0 = tx * 2 * kStemPoolCols - 1;               // the strip's first stem column
  const size_t hw = (size_t)a.H * a.W;
  const __amdgpu_buffer_rsrc_t xrsrc =
      U8 ? __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.x_u8 + (size_t)n * 3 * hw), 0, (int)(3 * hw), 0x00020000)
         : __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x + (size_t)n * 3 * hw), 0, (int)(3 * hw * sizeof(float)), 0x00020000);

  {
    const u32x4* wsrc = reinterpret_cast<const u32x4*>(a.w);
#pragma unroll
    for (int k = 0; k < kStemSteps; ++k) wl[tid + 256 * k] = wsrc[tid + 256 * k];
  }
  if (tid < 2 * kHsCout) {
    const int c = tid & (kHsCout - 1);
    ss[tid] = a.scale == nullptr ? (tid < kHsCout ? 1.f : 0.f) : (tid < kHsCout ? a.scale[c] : a.shift[c]);
  }
  const int r0 = tid / 35, pp = tid - r0 * 35;              // staging geometry (StemStager)
  const int ix = 2 * sx0 - 3 + 2 * pp;
  StemStager<U8> sg;
  const u32x4* wa0 = wl + khalf * 64 + l31;
  const uint32_t* pb0 = patch + wave * 4 * (kStemPP / 2) + l31;           // stem row 2 w of the band: patch row 4 w

  const int PHo = (a.OH - 1) / 2 + 1, PWo = (a.OW - 1) / 2 + 1;
  const size_t img = (size_t)n * a.Cout * PHo * PWo;
  const uint32_t plane_ob = (uint32_t)(PHo * PWo) * (uint32_t)sizeof(float);
  const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(a.y + img, 0, (int)(a.Cout * plane_ob), 0x00020000);
  constexpr uint32_t kOutside = 0xC0000000u;
  const int sx = sx0 + l31, pq = tx * kStemPoolCols + (l31 >> 1);
  const bool col_in = sx >= 0 && sx < a.OW;
  const bool col_st = (l31 & 1) != 0 && l31 < 2 * kStemPoolCols && pq < PWo;   // lane 2i + 1: centre of pooled column i
  // this lane's exchange word of register 0 in wave w's slot: + w * 1024, register j at + 32 j
  float* xl = xch + khalf * 16 + (l31 >> 1);

#ifdef ADX_HS_TRACE
  // phase totals of this workgroup (tools/stem_trace.py); its records sit behind those of the 3x3 kernel
  long long tr_c = 0, tr_e = 0, tr_s = 0, tr_t = 0;
  unsigned long long* tr = g_hs_trace + (size_t)(8192 + (blockIdx.x & 8191)) * 8;
  if (threadIdx.x == 0) tr[0] = __builtin_readcyclecounter();
#endif
  sg.load(a, xrsrc, r0, ix, b_begin * 16 - 3);
  sg.store(patch, r0, pp);
  __syncthreads();
#ifdef ADX_HS_TRACE
  if (threadIdx.x == 0) tr[1] = __builtin_readcyclecounter();
#endif
  float vm[32];                       // running maximum of this wave's pooled row (wave 0: carried in from the band above)
#pragma unroll
  for (int j = 0; j < 32; ++j) vm[j] = -INFINITY;
  float oamax = 0.f;                  // max |x| over the stored pooled values (the input's: sg.amax)
  for (int b = b_begin; b < b_end; ++b) {
#ifdef ADX_HS_TRACE
    tr_t = (long long)__builtin_readcyclecounter();
#endif
    const bool pre = b < b_own;       // the band in front of a segment: only its last odd row is wanted
    if (b + 1 < b_end) sg.load(a, xrsrc, r0, ix, (b + 1) * 16 - 3);
    // one stem row: the even one (rr = 0), then the odd one (rr = 1: also parked for pooled row p + 1).  Two straight-line
    // copies: a runtime rr splits the epilogue at every parked value and serialises its LDS reads.
    auto stem_row = [&](auto odd) {
      constexpr int rr = decltype(odd)::value ? 1 : 0;
      f32x16 accm[2], accl[2];
      stem_tile(wa0, pb0 + rr * 2 * (kStemPP / 2), khalf, accm, accl);
      // BN + ReLU; rows / columns outside the stem map are the pool's padding; then the horizontal maximum.  ReLU and padding as
      // min(max(t, 0), hi) with hi = +inf inside, -inf outside (v_max returns 0 for a NaN t)
      const int oy = b * 8 + 2 * wave + rr;
      const float hi = oy < a.OH && col_in ? INFINITY : -INFINITY;
      float hv[32];
#pragma unroll
      for (int half = 0; half < 2; ++half)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int cl = half * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
          float t = (accm[half][r] + accl[half][r] * (1.f / kLoScale)) * ss[cl] + ss[kHsCout + cl];
          t = __builtin_fminf(__builtin_fmaxf(t, 0.f), hi);
          // neighbours by DPP wavefront shifts; lanes whose shift crosses a 32-lane group are not pooled-column centres
          const int ti = __builtin_bit_cast(int, t);
          const float left = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(ti, 0x138 /* wave_shr:1 */, 0xf, 0xf, true));
          const float right = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(ti, 0x130 /* wave_shl:1 */, 0xf, 0xf, true));
          const int j = half * 16 + r;
          hv[j] = __builtin_fmaxf(__builtin_fmaxf(left, t), right);
          vm[j] = __builtin_fmaxf(vm[j], hv[j]);
        }
      if constexpr (rr == 1) {        // the odd row, for pooled row p + 1: written by the pooled-column centres
        if (l31 & 1) {
#pragma unroll
          for (int j = 0; j < 32; ++j) xl[wave * 1024 + 32 * j] = hv[j];
        }
      }
    };
    if (!pre) stem_row(std::false_type{});
    stem_row(std::true_type{});
#ifdef ADX_HS_TRACE
    { const long long t = (long long)__builtin_readcyclecounter(); tr_c += t - tr_t; tr_t = t; }
#endif
    __syncthreads();                  // odd rows parked; every wave is done with the patch
    {
      const float* src = xl + ((wave + 3) & 3) * 1024;
      float up[32];
#pragma unroll
      for (int j = 0; j < 32; ++j) up[j] = src[32 * j];
      if (wave != 0) {
#pragma unroll
        for (int j = 0; j < 32; ++j) vm[j] = __builtin_fmaxf(up[j], vm[j]);
      }
      const int pr = b * 4 + wave;
      if (!pre && pr < PHo) {
        const bool st = col_st;
        if (!a.y_cells) {
          const uint32_t voff = st ? (uint32_t)(pr * PWo + pq) * 4u + (uint32_t)(4 * khalf) * plane_ob : kOutside;
#pragma unroll
          for (int half = 0; half < 2; ++half)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int cu = half * 32 + (r & 3) + 8 * (r >> 2);       // + 4 * khalf, which rides in voff
              oamax = fp16_amax(oamax, st ? vm[half * 16 + r] : 0.f);     // (a lane that stores nothing may hold -inf)
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, vm[half * 16 + r]), yrsrc, voff, cu * plane_ob, 0);
            }
        } else {      // the pooled map as a cell tensor (conv2d_hs3x3_kernel: XCELLS): layer1's first conv copies cells
          const uint32_t cplane = (uint32_t)(PHo * PWo) * 16u;
          const uint32_t vcell = st ? (uint32_t)(pr * PWo + pq) * 16u + (uint32_t)khalf * 2u * cplane : kOutside;
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            float mm[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) mm[r] = st ? vm[half * 16 + r] : 0.f;     // (stores of !st lanes are dropped)
            cells_store32<false>(mm, nullptr, nullptr, 0, nullptr, false, yrsrc, vcell, (uint32_t)(half * 4) * 2u * cplane, cplane, oamax);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 32; ++j) vm[j] = wave == 0 ? up[j] : -INFINITY;
    }
#ifdef ADX_HS_TRACE
    { const long long t = (long long)__builtin_readcyclecounter(); tr_e += t - tr_t; tr_t = t; }
#endif
    if (b + 1 < b_end) sg.store(patch, r0, pp);
    __syncthreads();
#ifdef ADX_HS_TRACE
    { const long long t = (long long)__builtin_readcyclecounter(); tr_s += t - tr_t; tr_t = t; }
#endif
  }
#ifdef ADX_HS_TRACE
  if (threadIdx.x == 0) {
    tr[2] = (unsigned long long)tr_c;
    tr[3] = (unsigned long long)tr_e;
    tr[4] = (unsigned long long)tr_s;
    tr[5] = __builtin_readcyclecounter();
  }
#endif
  range_flag(a.status, out_of_fp16(fp16_amax(sg.amax, oamax)));
}

// [64][3][7][7] fp32 -> [step][plane][k-half][64][8] fp16 with k = (combo = 2*step + k-half -> channel combo/7,
// kernel row combo%7; element j = kernel column, the 8th and the 22nd combo are zero)
__global__ void conv2d_hs_stem_pack_kernel(const float* __restrict__ w, _Float16* __restrict__ p, uint32_t* status) {
  const int idx = blockIdx.x * 256 + threadIdx.x;      // over [step][k-half][64][8]
  if (idx >= kStemSteps * 2 * 64 * 8) return;
  const int j = idx & 7, ml = (idx >> 3) & 63, h = (idx >> 9) & 1, step = idx >> 10;
  const int combo = 2 * step + h;
  float v = 0.f;
  if (combo < 21 && j < 7) v = w[((size_t)ml * 3 + combo / 7) * 49 + (combo % 7) * 7 + j];
  const _Float16 hi = (_Float16)v;
  const _Float16 lo = (_Float16)((v - (float)hi) * kLoScale);
  const size_t cell = ((size_t)(step * 2 + 0) * 2 + h) * 64 + ml;
  p[cell * 8 + j] = hi;
  p[(cell + 128) * 8 + j] = lo;
  range_flag(status, out_of_fp16(v));
}

static bool hs_is_stem(const ConvSpec& L) { return L.k == 7 && L.stride == 2 && L.pad == 3 && L.cin == 3 && L.cout == 64; }

// fp32 [M][Kc][taps] (forward: M = cout, Kc = cin) or its data-gradient view (dgrad: M = original cin,
// Kc = original cout, taps flipped) -> [M/64][Kc/16][tap][plane][k-half][64][8] fp16
__global__ void conv2d_hs_pack_kernel(const float* __restrict__ w, _Float16* __restrict__ p, int M, int Kc, int Kreal,
                                      int taps, int dgrad, size_t total, uint32_t* status) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;   // over [M/64][Kc/16][tap][k-half][64][8]
  if (idx >= total) return;
  const int j = idx & 7;
  const int ml = (idx >> 3) & 63;
  const int h = (idx >> 9) & 1;
  size_t rest = idx >> 10;
  const int tap = rest % taps; rest /= taps;
  const int nchunks = Kc / kHsCC;
  const int chunk = rest % nchunks;
  const int ct = rest / nchunks;
  const int m = ct * 64 + ml, kc = chunk * kHsCC + h * 8 + j;
  float v = 0.f;
  if (kc < Kreal) v = dgrad ? w[((size_t)kc * M + m) * taps + (taps - 1 - tap)] : w[((size_t)m * Kreal + kc) * taps + tap];
  const _Float16 hi = (_Float16)v;
  const _Float16 lo = (_Float16)((v - (float)hi) * kLoScale);
  const size_t cell = ((((size_t)(ct * nchunks + chunk) * taps + tap) * 2 + 0) * 2 + h) * 64 + ml;
  p[cell * 8 + j] = hi;
  p[(cell + 128) * 8 + j] = lo;     // plane 1 is 2 * 64 cells further
  range_flag(status, out_of_fp16(v));
}

// The same for up to kHsPackJobs weight tensors in ONE launch (the training step re-lays every conv weight every step: 36
// forward images and 29 data-gradient images, each a ~5 us launch of its own otherwise).  The job table travels in the kernel
// arguments; a block finds its job by a binary search of the (wave-uniform) first-block column.
constexpr int kHsPackJobs = 48;
struct HsPackTable {
  const float* w[kHsPackJobs];
  _Float16* p[kHsPackJobs];
  int M[kHsPackJobs], Kc[kHsPackJobs], Kreal[kHsPackJobs], taps[kHsPackJobs], dgrad[kHsPackJobs];
  unsigned first[kHsPackJobs + 1];     // first block of job j; first[n] = the grid
  int n;
};
__global__ void __launch_bounds__(256) conv2d_hs_pack_many_kernel(const HsPackTable t) {
  int j = 0, jend = t.n;               // binary search of the job: six kernel-argument reads, not one per job
  while (jend - j > 1) {
    const int mid = (j + jend) >> 1;
    if (blockIdx.x >= t.first[mid]) j = mid; else jend = mid;
  }
  const int M = t.M[j], Kc = t.Kc[j], Kreal = t.Kreal[j], taps = t.taps[j], dgrad = t.dgrad[j];
  const float* __restrict__ w = t.w[j];
  _Float16* __restrict__ p = t.p[j];
  const size_t total = (size_t)M * Kc * taps;
  const size_t idx = (size_t)(blockIdx.x - t.first[j]) * 256 + threadIdx.x;   // over [M/64][Kc/16][tap][k-half][64][8]
  if (idx >= total) return;
  const int e = idx & 7;
  const int ml = (idx >> 3) & 63;
  const int h = (idx >> 9) & 1;
  size_t rest = idx >> 10;
  const int tap = rest % taps; rest /= taps;
  const int nchunks = Kc / kHsCC;
  const int chunk = rest % nchunks;
  const int ct = rest / nchunks;
  const int m = ct * 64 + ml, kc = chunk * kHsCC + h * 8 + e;
  float v = 0.f;
  if (kc < Kreal) v = dgrad ? w[((size_t)kc * M + m) * taps + (taps - 1 - tap)] : w[((size_t)m * Kreal + kc) * taps + tap];
  const _Float16 hi = (_Float16)v;
  const _Float16 lo = (_Float16)((v - (float)hi) * kLoScale);
  const size_t cell = ((((size_t)(ct * nchunks + chunk) * taps + tap) * 2 + 0) * 2 + h) * 64 + ml;
  p[cell * 8 + e] = hi;
  p[(cell + 128) * 8 + e] = lo;
}

int conv2d_hs_pack_many(const HsPackJob* jobs, int n, hipStream_t s) {
  for (int j0 = 0; j0 < n; j0 += kHsPackJobs) {
    HsPackTable t;
    t.n = std::min(kHsPackJobs, n - j0);
    unsigned blocks = 0;
    for (int j = 0; j < t.n; ++j) {
      const HsPackJob& q = jobs[j0 + j];
      ADX_REQUIRE(q.w != nullptr && q.packed != nullptr && q.cin_pad % kHsCC == 0 && q.cout % kHsCout == 0,
                  "conv2d_hs_pack_many: job %d is not a split-fp16 weight image", j0 + j);
      t.w[j] = q.w; t.p[j] = (_Float16*)q.packed;
      t.M[j] = q.cout; t.Kc[j] = q.cin_pad; t.Kreal[j] = q.cin; t.taps[j] = q.taps; t.dgrad[j] = q.dgrad;
      t.first[j] = blocks;
      blocks += (unsigned)(((size_t)q.cout * q.cin_pad * q.taps + 255) / 256);
    }
    t.first[t.n] = blocks;
    conv2d_hs_pack_many_kernel<<<dim3(blocks), dim3(256), 0, s>>>(t);
    ADX_LAUNCH_CHECK();
  }
  return ADX_OK;
}

static bool hs_eligible(const ConvSpec& L, const DebugSwitches& sw) {
  if (sw.conv_exact) return false;     // ADX_CONV_EXACT=1: every conv on the exact-fp32 MFMA kernels
  if (hs_is_stem(L) && !L.dgrad) return true;
  if (L.cin % kHsCC != 0 || L.cin_pad != L.cin || L.cout % kHsCout != 0) return false;
  return L.k == 3 && (L.stride == 1 || L.stride == 2);
}
bool conv2d_hs_eligible(const ConvSpec& L, const DebugSwitches& sw) { return hs_eligible(L, sw); }

size_t conv2d_packed_floats(const ConvSpec& L) {
  const size_t direct = (size_t)L.k * L.k * L.cin_pad * L.cout;
  return direct;
}

bool conv2d_hs_pack_batchable(const ConvSpec& c, int dgrad) { return conv2d_hs_eligible(c) && !(hs_is_stem(c) && !dgrad); }

int conv2d_hs_pack(const ConvSpec& c, const float* w, void* packed, int dgrad, hipStream_t s) {
  if (hs_is_stem(c) && !dgrad) {
    conv2d_hs_stem_pack_kernel<<<dim3(ceil_div(kStemSteps * 2 * 64 * 8, 256)), dim3(256), 0, s>>>(w, (_Float16*)packed, conv2d_status());
    ADX_LAUNCH_CHECK();
    return ADX_OK;
  }
  const size_t total = (size_t)c.cout * c.cin_pad * c.k * c.k;
  conv2d_hs_pack_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s>>>(
      w, (_Float16*)packed, c.cout, c.cin_pad, c.cin, c.k * c.k, dgrad, total, conv2d_status());
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

template <int STRIDE, int K, int ROWS, int PBUF, bool DS, bool XCELLS = false, bool YCELLS = false>
static int hs_launch_t(Conv2dArgs a, hipStream_t s) {
  constexpr int TH = 4 * ROWS;
  constexpr int PH = (TH - 1) * STRIDE + K, PW = (kTileW - 1) * STRIDE + K;
  constexpr size_t lds = (size_t)PBUF * 64 * PH * PW + (size_t)2 * K * 256 * 16 + (DS ? 256 * 16 : 0) +
                         (DS ? 4 : 2) * kHsCout * sizeof(float) + 16;
  static_assert(lds <= 80 * 1024, "two workgroups per CU need <= 80 KB each");
  static std::atomic<uint64_t> attr{0};
  if (DeviceOnce once{attr}; once) {
    ADX_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv2d_hs_kernel<STRIDE, K, ROWS, PBUF, DS, XCELLS, YCELLS>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    once.commit();
  }
  a.tiles_x = ceil_div(a.OW, kTileW); a.tiles_y = ceil_div(a.OH, TH); a.cout_tiles = a.Cout / kHsCout;
  const size_t grid = (size_t)a.cout_tiles * a.tiles_x * a.tiles_y * a.N;
  ADX_REQUIRE(grid < (1u << 31), "conv2d_hs: grid too large");
  ADX_REQUIRE((size_t)a.Cout * a.OH * a.OW * sizeof(float) < 0x7FFFFFFFu, "conv2d_hs: one image of the output exceeds the 32-bit byte offsets");
  conv2d_hs_kernel<STRIDE, K, ROWS, PBUF, DS, XCELLS, YCELLS><<<dim3((unsigned)grid), dim3(256), lds, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

static int hs_stem_launch(Conv2dArgs a, hipStream_t s) {
  constexpr size_t lds = (size_t)kStemSteps * 4096 + (size_t)2 * 4 * 3 * kStemPH * kStemPP + 2 * kHsCout * sizeof(float);
  static_assert(lds <= 80 * 1024, "two workgroups per CU need <= 80 KB each");
  static std::atomic<uint64_t> attr{0};
  if (DeviceOnce once{attr}; once) {
    ADX_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv2d_hs_stem_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds));
    once.commit();
  }
  a.tiles_x = ceil_div(a.OW, kTileW); a.cout_tiles = 1;
  a.tiles_y = ceil_div(a.OH, 8);
  // few images: split the bands' tile walks so that the grid covers the chip
  const int bands = a.tiles_y * a.N;
  a.stem_seg_tiles = 0; a.stem_nseg = 1;
  if (bands < 128 && a.tiles_x > 1) {
    const int want = std::min(a.tiles_x, std::max(1, 256 / bands));
    a.stem_seg_tiles = ceil_div(a.tiles_x, want);
    a.stem_nseg = ceil_div(a.tiles_x, a.stem_seg_tiles);
    if (a.stem_nseg <= 1) { a.stem_seg_tiles = 0; a.stem_nseg = 1; }
  }
  conv2d_hs_stem_kernel<<<dim3((unsigned)(bands * a.stem_nseg)), dim3(256), lds, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

template <bool U8>
static int hs_stem_pool_launch(Conv2dArgs a, hipStream_t s) {
  constexpr size_t lds = (size_t)kStemSteps * 4096 + (size_t)4 * 3 * kStemPH * kStemPP + 2 * kHsCout * sizeof(float) +
                         (size_t)4 * 1024 * sizeof(float);     // weights, one patch copy, BN, the four waves' parked odd rows
  static_assert(lds <= 80 * 1024, "two workgroups per CU need <= 80 KB each");
  static std::atomic<uint64_t> attr{0};
  if (DeviceOnce once{attr}; once) {
    ADX_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv2d_hs_stem_pool_kernel<U8>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    once.commit();
  }
  // strips of 15 pooled columns, bands of 4 pooled rows
  a.tiles_x = ceil_div((a.OW - 1) / 2 + 1, kStemPoolCols); a.cout_tiles = 1;
  a.tiles_y = ceil_div((a.OH - 1) / 2 + 1, 4);
  // few images: cut the strips' walks into segments of stem_seg_tiles bands so that the grid covers the chip (one 256x900
  // frame: 15 strips of 16 bands); a segment below the top recomputes one odd stem row per wave of the band above it
  const int strips = a.tiles_x * a.N;
  a.stem_seg_tiles = 0; a.stem_nseg = 1;
  if (strips < 256 && a.tiles_y > 1) {
    const int want = std::min(a.tiles_y, std::max(1, 512 / strips));
    a.stem_seg_tiles = ceil_div(a.tiles_y, want);
    a.stem_nseg = ceil_div(a.tiles_y, a.stem_seg_tiles);
    if (a.stem_nseg <= 1) { a.stem_seg_tiles = 0; a.stem_nseg = 1; }
  }
  conv2d_hs_stem_pool_kernel<U8><<<dim3((unsigned)(strips * a.stem_nseg)), dim3(256), lds, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

int conv2d_hs_stem_pool(const ConvSpec& L, const float* x, const float* w, const float* scale, const float* shift,
                        float* pooled, int N, int H, int W, hipStream_t s, const uint8_t* frames_u8, const float* mean,
                        const float* stdv, int y_cells) {
  ADX_REQUIRE((x || frames_u8) && w && scale && shift && pooled, "conv2d_hs_stem_pool: null pointer");
  ADX_REQUIRE((size_t)3 * H * W * sizeof(float) < 0xC0000000u, "conv2d_hs_stem_pool: image too large for 32-bit offsets");
  Conv2dArgs a{};
  a.x = x; a.w = w; a.scale = scale; a.shift = shift; a.y = pooled;
  if (frames_u8 != nullptr) {
    ADX_REQUIRE(mean && stdv, "conv2d_hs_stem_pool: uint8 frames need mean / std");
    a.x_u8 = frames_u8;
    for (int c = 0; c < 3; ++c) { a.u8_mean[c] = mean[c]; a.u8_std[c] = stdv[c]; }
  }
  a.N = N; a.Cin = 3; a.H = H; a.W = W; a.Cout = 64;
  a.OH = conv_out_dim(H, 7, 2, 3); a.OW = conv_out_dim(W, 7, 2, 3);
  a.KH = 7; a.KW = 7; a.stride = 2; a.pad = 3; a.relu = 1;
  a.cin_pad = L.cin_pad; a.cc = L.cc;
  a.y_cells = y_cells;
  a.status = conv2d_status();
  return frames_u8 != nullptr ? hs_stem_pool_launch<true>(a, s) : hs_stem_pool_launch<false>(a, s);
}

int conv2d_hs_launch_block_s2(const ConvSpec& c1, const ConvSpec& ds, const float* x, const float* w1, const float* scale1,
                              const float* shift1, float* y1, const float* wd, const float* scaled, const float* shiftd,
                              float* yd, int N, int H, int W, hipStream_t s, int x_cells, int y_cells, int relu, bool force_32) {
  ADX_REQUIRE(x && w1 && y1 && wd && yd && (scale1 != nullptr) == (shift1 != nullptr) && (scaled != nullptr) == (shiftd != nullptr),
              "conv2d_hs block launch: null pointer");
  Conv2dArgs a{};
  a.x = x; a.w = w1; a.scale = scale1; a.shift = shift1; a.res = nullptr; a.y = y1; a.x_amax = nullptr; a.x_amax_n = 0;
  a.w_ds = wd; a.scale_ds = scaled; a.shift_ds = shiftd; a.y_ds = yd;
  a.N = N; a.Cin = c1.cin; a.H = H; a.W = W; a.Cout = c1.cout;
  a.OH = conv_out_dim(H, 3, 2, 1); a.OW = conv_out_dim(W, 3, 2, 1);
  a.KH = 3; a.KW = 3; a.stride = 2; a.pad = 1; a.relu = relu;
  a.cin_pad = c1.cin_pad; a.cc = c1.cc;
  a.x_cells = x_cells;
  a.y_cells = y_cells;
  a.status = conv2d_status();
  HsS2Query q;
  q.N = N; q.H = H; q.W = W; q.x_cells = x_cells != 0; q.y_cells = y_cells != 0;
  if (q.x_cells && q.y_cells && !force_32) {      // (the persistent grid of the 16x16x32 kernel)
    const int rc = launch_cus(&q.cus);
    if (rc != ADX_OK) return rc;
    const HsS2Plan plan = conv2d_hs_s2_plan(c1, ds, q);
    if (plan.q) return conv2d_hs3x3q_s2_launch(plan, a, s);
  }
  return conv2d_hs_launch(c1, a, s);
}

HsS2Plan conv2d_hs_s2_plan(const ConvSpec& c1, const ConvSpec& ds, const HsS2Query& q, const DebugSwitches& sw) {
  HsS2Plan p;
  const bool shape = hs_eligible(c1, sw) && c1.k == 3 && c1.stride == 2 && c1.pad == 1 && ds.k == 1 && ds.stride == 2 && ds.pad == 0 &&
                     ds.cin == c1.cin && ds.cout == c1.cout && c1.cin_pad % 64 == 0 && c1.cout % 128 == 0;
  if (!shape || !q.x_cells || !q.y_cells || !sw.hs_s2q || !sw.hs_dma || sw.hs_mode >= 0 || q.N < 1 || q.H < 1 || q.W < 1) return p;
  const int N = q.N, OH = conv_out_dim(q.H, 3, 2, 1), OW = conv_out_dim(q.W, 3, 2, 1);
  // one descriptor with 32-bit offsets per tensor, and the virtual row's division (conv2d_hs3x3_plan)
  if ((size_t)N * c1.cin * q.H * q.W * sizeof(float) >= 0xC0000000u || (size_t)N * c1.cout * OH * OW * sizeof(float) >= 0xC0000000u ||
      (long)N * (OW + 1) >= (1L << 21))
    return p;
  p.q = true;
  p.vw = N > 1 ? OW + 1 : OW;
  p.tiles_x = (int)(((long)N * p.vw - (N > 1 ? 1 : 0) + kTileW - 1) / kTileW);
  p.tiles_y = ceil_div(OH, kQTH);
  p.cout_tiles = c1.cout / 128;
  // workgroup = (XCD, slot), as for the stride-1 launches of the kernel: one workgroup per CU the launch may use where the units allow
  p.q_slots = hs3x3q_slots(p.cout_tiles * p.tiles_x * p.tiles_y, q.cus, sw.hs_persist);
  p.grid = (size_t)8 * p.q_slots;
  p.threads = kQNT;
  p.lds = kQLdsS2;
  return p;
}

// second half of a split 3x3 conv: y = [relu](sum_p part[p] * scale[c] + shift[c] [+ res]), four elements per thread
// (parts are added in index order: deterministic)
__global__ void __launch_bounds__(256) conv2d_split_reduce_kernel(const float* __restrict__ part, size_t part_stride, int nparts,
                                                                  const float* __restrict__ scale, const float* __restrict__ shift,
                                                                  const float* __restrict__ res, float* __restrict__ y,
                                                                  int cout, int plane4, size_t total4, int relu, uint32_t* status) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;      // (a whole wave, or the tail lanes of the last one: range_flag's ballot skips them)
  const int c = (int)((i / plane4) % cout);
  f32x4 v = reinterpret_cast<const f32x4*>(part)[i];
  for (int p0 = 1; p0 < nparts; p0 += 8) {        // eight loads in flight, added in index order
    f32x4 t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = reinterpret_cast<const f32x4*>(part + (size_t)(p0 + j < nparts ? p0 + j : 0) * part_stride)[i];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (p0 + j < nparts) v += t[j];
  }
  const float sc = scale != nullptr ? scale[c] : 1.f, sh = shift != nullptr ? shift[c] : 0.f;
  v = v * sc + sh;
  if (res != nullptr) v += reinterpret_cast<const f32x4*>(res)[i];
  if (relu) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = __builtin_fmaxf(v[k], 0.f);
  }
  reinterpret_cast<f32x4*>(y)[i] = v;
  float amax = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) amax = fp16_amax(amax, v[k]);
  range_flag(status, out_of_fp16(amax));
}

// LDS bytes of conv2d_hs3x3_kernel<MODE, STATS>: the patch and weight buffers, the BN constants (STATS == 2: + the consumer BatchNorm's)
static constexpr size_t hs3x3_lds(int mode, int stats, bool pair = false) {
  const int th = mode == 1 ? 16 : 8, ct = mode == 2 ? 2 : 1;
  const size_t patch = pair ?(size_t)2 * 2 * kHsPairKHalf * 16 : (size_t)2 * 64 * (th + 2) * 34;     // two copies of two k-halves
  return patch + (size_t)2 * (pair ? 2 : 3 * ct) * 256 * 16 + (2 * 64 * ct + 8) * sizeof(float) + 48 +
         (stats == 2 ? 4 * 64 * ct * sizeof(float) : 0);
}
static_assert(hs3x3_lds(0, 2) <= 80 * 1024 && hs3x3_lds(1, 2) <= 160 * 1024 && hs3x3_lds(2, 2) <= 160 * 1024, "LDS budget");
static_assert(hs3x3_lds(0, 0, true) <= 80 * 1024, "LDS budget: two workgroups of the PAIR form per CU");

Hs3x3Plan conv2d_hs3x3_plan(const ConvSpec& L, const Hs3x3Query& q, const DebugSwitches& sw) {
  Hs3x3Plan p;
  p.admitted = q.fmt == 0;
  if (!hs_eligible(L, sw) || !(L.k == 3 && L.stride == 1 && L.pad == 1) || (L.cin_pad / kHsCC) % 2 != 0) return p;
  const int N = q.N, OH = q.H, OW = q.W, nchunks = L.cin_pad / kHsCC;      // (pad 1: the output has the input's size)
  // The three tiles time within 3 % of each other on every ResNet-34 shape (the MFMA rate the chip sustains on
  // random data paces all of them): short K loops take the small tile (better tail balance), long ones the
  // 8-wave tiles that move fewer operand bytes per MFMA.
  int mode = L.cin < 256 ? 0 : (OH > 8 ? 1 : (L.cout % 128 == 0 ? 2 : 0));
  // small batches (the deployed case: one camera frame per tick): the 8-wave tiles leave most of the chip idle (512->512
  // @8x29 at B = 1: four workgroups); the 4-wave tile doubles the workgroup count
  const long grid0 = (long)N * ceil_div(OH, 8) * ceil_div(OW, kTileW) * (L.cout / kHsCout);      // mode 0's grid
  if (grid0 <= 256) mode = 0;
  if (sw.hs_mode >= 0 && !(sw.hs_mode == 2 && L.cout % 128 != 0)) mode = sw.hs_mode == 1 || sw.hs_mode == 2 ? sw.hs_mode : 0;   // ADX_HS_MODE pins it
  const int th = mode == 1 ? 16 : 8, ct = mode == 2 ? 2 : 1;
  const bool xc = (q.fmt & kFmtXCells) != 0, yc = (q.fmt & kFmtYCells) != 0, rc = (q.fmt & kFmtResCells) != 0 && q.has_res;
  const bool xscaled = q.x_scale == kXScalePre;
  // the cell kernels and the virtual row address whole tensors through one descriptor with 32-bit offsets (batches of ~870 frames
  // at 256x900 and up stay on the fp32 layout with its per-image descriptors)
  const bool in_ok = (size_t)N * L.cin * q.H * q.W * sizeof(float) < 0xC0000000u;
  const bool bytes_ok = in_ok && (size_t)N * L.cout * OH * OW * sizeof(float) < 0xC0000000u;
  // the virtual row: column tiles over the images side by side, one shared zero column between neighbours (the last one's needs no tile)
  const bool vfits = (long)N * (OW + 1) < (1L << 21);
  const int vw = N > 1 ? OW + 1 : OW;
  const int vtiles_x = (int)(((long)N * vw - (N > 1 ? 1 : 0) + kTileW - 1) / kTileW);
  const bool vrow_ok = sw.conv_vrow && N > 1 && vfits && bytes_ok;     // fp32-layout launches of a whole batch tile it too
  // the 16x16x32 kernel where its tile rules hold: plain cell launches, the training forward on a cell input (TRAIN == 1), a data
  // gradient with the consumer BatchNorm's sums on cells under their scale (TRAIN == 2)
  const bool q_shape = sw.hs_mode < 0 && L.cout % 128 == 0 && L.cin_pad % 64 == 0;
  const bool q_fp32out = q_shape && xc && !yc && !rc && !q.affine && vfits && bytes_ok;
  const bool q_train = q_fp32out && sw.train_cells >= 3 && !q.has_res && q.x_scale == kXScaleNone && q.bst_mask == 0;
  const bool q_dgrad = q_fp32out && sw.train_cells >= 5 && xscaled && !q.relu && (q.bst_mask == 2 || (q.bst_mask == 1 && q.bst_bits));
  const bool q_plain = q_shape && xc && yc && (!q.has_res || rc) && q.x_scale == kXScaleNone;
  // statistics: one slot per workgroup of the launch that would leave them, taken when the buffer on offer holds them
  const int stats_tiles = q_train || q_dgrad ? ceil_div(OH, kQTH) * vtiles_x
                                             : ceil_div(OH, th) * (!yc && !rc && vrow_ok ? vtiles_x : N * ceil_div(OW, kTileW));
  p.stats_need = (size_t)stats_tiles * (L.cout * 2 + L.cout / 64);
  const bool stats = q.stats_floats > 0 && p.stats_need <= q.stats_floats;
  // cells belong to the INPUT of a training-forward launch, to the input of a data gradient written under a known power-of-two
  // scale, or to plain launches (the inference executor: no statistics, no split reduction)
  const bool split_shape = mode == 0 && grid0 <= 64 && nchunks >= 8;
  if (q.fmt == kFmtXCells && q.stats_floats > 0 && q.bst_mask == 0 && q.x_scale == kXScaleNone && sw.train_cells != 0 && !L.dgrad)
    p.admitted = in_ok && stats;
  else if (q.fmt == (kFmtXCells | kFmtXScaled) && L.dgrad && xscaled && sw.train_cells >= 4)
    p.admitted = in_ok;
  else if (q.fmt != 0)
    p.admitted = q.stats_floats == 0 && sw.conv_cells && !L.dgrad && bytes_ok && !split_shape;

  p.family = kHs3x3; p.mode = mode; p.threads = mode == 0 ? 256 : 512;
  p.tiles_x = ceil_div(OW, kTileW); p.tiles_y = ceil_div(OH, th); p.cout_tiles = L.cout / (kHsCout * ct);
  p.vw = OW; p.cper = nchunks;
  p.grid = (size_t)p.cout_tiles * p.tiles_x * p.tiles_y * N;
  if (stats) { p.stats = q.bst_mask != 0 ? 2 : 1; p.stats_tiles = stats_tiles; }
  // Small batches (one camera frame per tick): a 512->512 layer on one 8x29 map is 8 workgroups, each walking 96 stages
  // (83 us); with a scratch buffer the chunks are split over up to 16 workgroups per tile and a reduce launch finishes.
  if (!stats && split_shape && q.split_floats > 0 && q.x_scale == kXScaleNone && (OH * OW) % 4 == 0 && q.y_aligned && (!q.has_res || q.res_aligned)) {
    const size_t out_floats = (size_t)N * L.cout * OH * OW;
    int S = 16;
    while (S > 1 && (nchunks % S != 0 || (nchunks / S) % 2 != 0 || p.grid * S > 256 || out_floats * S > q.split_floats)) S >>= 1;
    if (S > 1) { p.ksplit = S; p.cper = nchunks / S; p.grid *= S; }
  }
  // a data gradient (no statistics wanted from it) on a gradient that was written as cells has an fp32 output [+ fp32 residual];
  // any other cell operand comes with a cell output: the executor keeps a layer's 3x3 convs in the cell layout from the first
  // one's output to the last one's (the stride-2 kernel and the average pool read cells too)
  const bool cells_out = !stats && p.ksplit == 1 && (xc || yc || rc) && !(xc && xscaled && !yc && !rc);
  if (stats ? q_train || q_dgrad : cells_out && q_plain) {
    p.family = kHs3x3q; p.dma = sw.hs_dma; p.threads = kQNT;
    p.lds = p.dma ? kQLdsD : kQLds;
    p.vw = vw; p.tiles_x = vtiles_x; p.tiles_y = ceil_div(OH, kQTH); p.cout_tiles = L.cout / 128;
    // workgroup = (XCD, slot); slots per XCD: as many as the longest eighth of the units (spatial tile, cout tile) (one unit per
    // workgroup: ADX_HS_PERSIST=0 and the register-staged form), or -- the LDS-DMA form -- one workgroup per CU the launch may
    // use (q.cus: the device's less a reserve), each walking its XCD's range in steps of that count (bit-identical results either way)
    p.q_slots = hs3x3q_slots(p.cout_tiles * p.tiles_x * p.tiles_y, q.cus, sw.hs_dma && sw.hs_persist);
    p.grid = (size_t)8 * p.q_slots;
    return p;
  }
  // the PAIR form: every plain launch of the 4-wave tile, whatever its operand formats (a rule on the formats would give the fp32
  // and the cell launch of one conv different summation orders); ADX_HS_MODE pins the 32x32x16 code
  p.pair = sw.hs_pair && sw.hs_mode < 0 && mode == 0 && p.ksplit == 1 && !stats;
  p.lds = hs3x3_lds(mode, p.stats, p.pair);
  if (p.ksplit > 1) return p;
  p.xcells = xc; p.ycells = cells_out;
  p.vr = !cells_out && (!(xc || yc || rc) || ((stats || xscaled) && !yc && !rc)) && vrow_ok;
  if (p.ycells || p.vr) {
    p.vw = vw; p.tiles_x = vtiles_x;
    p.grid = (size_t)p.cout_tiles * p.tiles_x * p.tiles_y;
  }
  return p;
}

typedef void (*HsKernel)(const Conv2dArgs);

// every instantiation of conv2d_hs3x3_kernel of one tile mode, at [((STATS * 2 + XCELLS) * 2 + YCELLS) * 2 + VR] (null: there is none)
template <int MODE>
static const HsKernel* hs3x3_kernels() {
#define HS_K(S, X, Y, V) &conv2d_hs3x3_kernel<MODE, S, X, Y, V>
  static const HsKernel table[3 * 8] = {
      HS_K(0, false, false, false), HS_K(0, false, false, true), HS_K(0, false, true, false), nullptr,
      HS_K(0, true, false, false),  HS_K(0, true, false, true),  HS_K(0, true, true, false),  nullptr,
      HS_K(1, false, false, false), HS_K(1, false, false, true), nullptr, nullptr,
      HS_K(1, true, false, false),  HS_K(1, true, false, true),  nullptr, nullptr,
      HS_K(2, false, false, false), HS_K(2, false, false, true), nullptr, nullptr,
      HS_K(2, true, false, false),  HS_K(2, true, false, true),  nullptr, nullptr};
#undef HS_K
  return table;
}

// the PAIR instantiations (MODE 0, STATS 0), at the same index
static const HsKernel* hs3x3_pair_kernels() {
#define HS_K(X, Y, V) &conv2d_hs3x3_kernel<0, 0, X, Y, V, true>
  static const HsKernel table[8] = {HS_K(false, false, false), HS_K(false, false, true), HS_K(false, true, false), nullptr,
                                    HS_K(true, false, false),  HS_K(true, false, true),  HS_K(true, true, false),  nullptr};
#undef HS_K
  return table;
}

static int hs3x3_launch(const Hs3x3Plan& p, Conv2dArgs a, hipStream_t s) {
  const HsKernel* const table = p.pair ? hs3x3_pair_kernels() : (p.mode == 1 ? hs3x3_kernels<1>() : (p.mode == 2 ? hs3x3_kernels<2>() : hs3x3_kernels<0>()));
  static std::atomic<uint64_t> attr[4];
  if (DeviceOnce once{attr[p.pair ? 3 : p.mode]}; once) {
    for (int v = 0; v < (p.pair ? 8 : 3 * 8); ++v)
      if (table[v] != nullptr)
        ADX_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(table[v]), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)hs3x3_lds(p.mode, v / 8, p.pair)));
    once.commit();
  }
  ADX_REQUIRE(!p.pair || (p.mode == 0 && p.stats == 0 && p.ksplit == 1), "conv2d_hs: the PAIR form is the plain 4-wave tile (internal error)");
  ADX_REQUIRE(p.grid < (1u << 31), "conv2d_hs: grid too large");
  ADX_REQUIRE((size_t)a.Cout * a.OH * a.OW * sizeof(float) < 0x7FFFFFFFu, "conv2d_hs: one image of the output exceeds the 32-bit byte offsets");
  if (p.ycells) {
    ADX_REQUIRE(a.y_cells && a.x_amax == nullptr, "conv2d_hs: cell-layout operands come with a cell-layout output (and no dynamic range)");
    ADX_REQUIRE((long)a.N * p.vw < (1L << 21), "conv2d_hs: batch x width exceeds the virtual-row arithmetic");
    ADX_REQUIRE((size_t)a.N * a.Cout * a.OH * a.OW * sizeof(float) < 0xC0000000u && (size_t)a.N * a.Cin * a.H * a.W * sizeof(float) < 0xC0000000u,
                "conv2d_hs: a cell-layout tensor exceeds the 32-bit byte offsets");
  } else if (p.xcells) {
    // training forward on a cell-layout input (resnet_train.hip: the activation between a block's two convs): the staging copies
    // cells instead of converting fp32 values, everything else -- fp32 conv output, statistics -- as for an fp32 input
    // ... or a data gradient reading a gradient that was written as cells, with or without the consumer BatchNorm's sums
    ADX_REQUIRE(p.stats == 0 || ((a.x_amax == nullptr || a.x_amax_n < 0) && (a.bs_raw == nullptr) == (a.x_amax == nullptr) && !a.y_cells && !a.res_cells),
                "conv2d_hs: a cell-layout input with statistics belongs to a training-forward launch or to a data gradient with its scale");
    ADX_REQUIRE((size_t)a.N * a.Cin * a.H * a.W * sizeof(float) < 0xC0000000u, "conv2d_hs: a cell-layout tensor exceeds the 32-bit byte offsets");
  }
  a.tiles_x = p.tiles_x; a.tiles_y = p.tiles_y; a.cout_tiles = p.cout_tiles;
  a.vw = p.vw; a.inv_vw = 1.f / (float)p.vw;
  a.ksplit = p.ksplit; a.cper = p.cper;
  const HsKernel kernel = table[((p.stats * 2 + p.xcells) * 2 + p.ycells) * 2 + p.vr];
  ADX_REQUIRE(kernel != nullptr, "conv2d_hs: no kernel variant for this plan (internal error)");
  const dim3 grid((unsigned)p.grid), block(p.threads);
  if (p.ksplit > 1) {       // the parts to the scratch, then a reduce launch with the epilogue
    const size_t out_floats = (size_t)a.N * a.Cout * a.OH * a.OW, total4 = out_floats / 4;
    Conv2dArgs c = a;
    c.part_stride = out_floats;
    c.scale = nullptr; c.shift = nullptr; c.res = nullptr; c.relu = 0; c.status = nullptr;
    kernel<<<grid, block, p.lds, s>>>(c);
    ADX_LAUNCH_CHECK();
    conv2d_split_reduce_kernel<<<dim3((unsigned)ceil_div((long)total4, 256L)), dim3(256), 0, s>>>(
        a.part, out_floats, p.ksplit, a.scale, a.shift, a.res, a.y, a.Cout, a.OH * a.OW / 4, total4, a.relu, a.status);
    ADX_LAUNCH_CHECK();
    return ADX_OK;
  }
  a.part = nullptr;
  kernel<<<grid, block, p.lds, s>>>(a);
  ADX_LAUNCH_CHECK();
  return ADX_OK;
}

// forward weight [cout][cin][3][3] -> weight [4 cin][cout][2][2] of the 2x2 conv that is the stride-2 data gradient:
// class (py, px), window cell (r, c) of dy -> the forward tap (kh, kw) that links them, or none.  Row rule (columns alike):
// an even input row 2j is reached from output row j through kh = 1 only (window row 0); an odd row 2j + 1 from output row j
// through kh = 2 (window row 0) and from output row j + 1 through kh = 0 (window row 1).
__global__ void dgrad_s2_weights_kernel(const float* __restrict__ w, float* __restrict__ out, int cin, int cout) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;     // over [4][cin][cout][2][2]
  if (idx >= (size_t)16 * cin * cout) return;
  const int c = idx & 1, r = (idx >> 1) & 1;
  size_t rest = idx >> 2;
  const int co = rest % cout; rest /= cout;
  const int ci = rest % cin;
  const int cls = (int)(rest / cin), py = cls >> 1, px = cls & 1;
  const int kh = py == 0 ? (r == 0 ? 1 : -1) : (r == 0 ? 2 : 0);
  const int kw = px == 0 ? (c == 0 ? 1 : -1) : (c == 0 ? 2 : 0);
  out[idx] = (kh >= 0 && kw >= 0) ? w[(((size_t)co * cin + ci) * 3 + kh) * 3 + kw] : 0.f;
}

bool conv2d_hs_dgrad_s2_eligible(int cin, int cout) {
  ConvSpec probe{};
  probe.cin = cout; probe.cin_pad = cout; probe.cout = 4 * cin; probe.k = 3; probe.stride = 1; probe.dgrad = 1;
  return cin % kHsCout == 0 && cout % kHsCC == 0 && conv2d_hs_eligible(probe);
}

int conv2d_hs_dgrad_s2(const float* w, const float* dy, float* dx, int accumulate, int N, int cin, int cout, int H, int W,
                       float* wbuild, float* wimg, const uint32_t* dy_amax, int dy_amax_n, hipStream_t s) {
  ADX_REQUIRE(w && dy && dx && wbuild && wimg, "conv2d_hs_dgrad_s2: null pointer");
  ADX_REQUIRE(conv2d_hs_dgrad_s2_eligible(cin, cout), "conv2d_hs_dgrad_s2: cin %d / cout %d outside the kernel's rules", cin, cout);
  const size_t nw = (size_t)16 * cin * cout;
  dgrad_s2_weights_kernel<<<dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s>>>(w, wbuild, cin, cout);
  ADX_LAUNCH_CHECK();
  ConvSpec g{};
  g.cin = cout; g.cin_pad = cout; g.cout = 4 * cin; g.k = 2; g.stride = 1; g.pad = 0; g.cc = kHsCC;
  int rc = conv2d_hs_pack(g, wbuild, wimg, 0, s);
  if (rc != ADX_OK) return rc;
  Conv2dArgs a{};
  a.x = dy; a.w = wimg; a.res = accumulate ? dx : nullptr; a.y = dx; a.x_amax = dy_amax; a.x_amax_n = dy_amax_n;
  a.N = N; a.Cin = cout; a.H = conv_out_dim(H, 3, 2, 1); a.W = conv_out_dim(W, 3, 2, 1); a.Cout = 4 * cin;
  a.OH = a.H; a.OW = a.W;                  // one 2x2 window per low-resolution pixel; the window's far row / column may lie
  a.KH = 2; a.KW = 2; a.stride = 1; a.pad = 0; a.relu = 0;     // outside dy: zeros, like any padding
  a.cin_pad = cout; a.cc = kHsCC;
  a.d2s_cin = cin; a.d2s_h = H; a.d2s_w = W;
  ADX_REQUIRE((size_t)cin * H * W * sizeof(float) < 0x7FFFFFFFu, "conv2d_hs_dgrad_s2: one image of dx exceeds the 32-bit byte offsets");
  return hs_launch_t<1, 2, 2, 2, false>(a, s);
}

int conv2d_hs_launch(const ConvSpec& L, Conv2dArgs a, hipStream_t s, const Hs3x3Plan* plan) {
  ADX_REQUIRE((size_t)L.cin * a.H * a.W * sizeof(float) < 0xC0000000u, "conv2d_hs: one image of the input exceeds the 32-bit byte offsets");
  const bool ds = a.w_ds != nullptr;
  if (hs_is_stem(L) && !ds) {
    ADX_REQUIRE(a.x_amax == nullptr && a.res == nullptr, "conv2d_hs stem: no residual / dynamic range");
    return hs_stem_launch(a, s);
  }
  if (L.k == 3 && L.stride == 1 && !ds) {
    if (plan != nullptr && plan->family != kHsNone) return plan->family == kHs3x3q ? conv2d_hs3x3q_launch(*plan, a, s) : hs3x3_launch(*plan, a, s);
    ADX_REQUIRE(a.stats_part == nullptr, "conv2d_hs: statistics requested from a launch the pipelined kernel does not serve");
    return hs_launch_t<1, 3, 2, 2, false>(a, s);
  }
  if (L.k == 3 && L.stride == 2 && L.pad == 1) {
    if (a.x_cells || a.y_cells) {
      ADX_REQUIRE(ds && a.x_amax == nullptr && a.res == nullptr && a.d2s_cin == 0,
                  "conv2d_hs: cell-layout operands of the stride-2 conv need the fused downsample launch (no residual, no dynamic range)");
      if (a.x_cells && a.y_cells) return hs_launch_t<2, 3, 1, 1, true, true, true>(a, s);
      return a.x_cells ? hs_launch_t<2, 3, 1, 1, true, true, false>(a, s) : hs_launch_t<2, 3, 1, 1, true, false, true>(a, s);
    }
    return ds ? hs_launch_t<2, 3, 1, 1, true>(a, s) : hs_launch_t<2, 3, 1, 1, false>(a, s);
  }
  set_error("conv2d_hs: no kernel for k=%d stride=%d pad=%d%s", L.k, L.stride, L.pad, ds ? " with a fused downsample" : "");
  return ADX_ERR_INVALID;
}

}  // namespace adx

#ifdef ADX_HS_TRACE
extern "C" int adx_hs_trace_read(unsigned long long* host, int nwords) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(adx::g_hs_trace), (size_t)nwords * 8);
}
#endif
