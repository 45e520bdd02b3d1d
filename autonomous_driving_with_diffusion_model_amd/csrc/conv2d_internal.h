// Shared between the inference (conv2d.hip) and training (resnet_train.hip) perception executors.
#pragma once
#include <algorithm>
#include <vector>

#include "adx_common.h"

namespace adx {

constexpr int kTileH = 4;    // output rows per workgroup (one per wave)
constexpr int kTileW = 32;   // output columns per workgroup (= MFMA N)

struct ConvSpec {
  int cin, cout, k, stride, pad;
  int t_w, t_g, t_b, t_m, t_v;           // tensor indices (weight, bn gamma, beta, mean, var)
  size_t o_w, o_scale, o_shift;          // float offsets in the packed buffer
  int cin_pad, cc;
  int fuse_with;                         // ResNet executor: index of the conv1 this downsample conv can ride on, or -1
  int dgrad;                             // 1: this launch is the data-gradient view of a forward conv
};

struct Conv2dArgs {
  const float* x;       // [N][Cin][H][W]
  const float* w;       // packed [KH*KW][cin_pad][Cout]
  const float* scale;   // [Cout] or null
  const float* shift;   // [Cout] or null
  const float* res;     // [N][Cout][OH][OW] or null
  float* y;             // [N][Cout][OH][OW]
  const float* w_ds;    // conv2d_hs only: fused 1x1 stride-2 downsample (packed weights, BN scale/shift, output) or null
  const float* scale_ds;
  const float* shift_ds;
  float* y_ds;
  const uint32_t* x_amax;  // optional: x_amax_n partial maxima of |x| as bit patterns (conv2d_hs rescales x by a power of two);
  int x_amax_n;            // x_amax_n < 0: x_amax points at two floats {xs, 1 / xs} instead -- the power of two a cell-layout x was
                           // ALREADY multiplied by when it was written (resnet_train.hip: bn_bwd_apply_groups_kernel)
  // stem only: the camera frames as uint8 [N][H][W][3]; ToTensor + Normalize ((v / 255 - mean) / std, the arithmetic of
  // image_normalize_kernel) happen in the staging load and the fp32 NCHW tensor is never written (x is unused then)
  const uint8_t* x_u8;
  float u8_mean[3], u8_std[3];
  int N, Cin, H, W, Cout, OH, OW, KH, KW, stride, pad, relu;
  int cin_pad, cc;      // channels padded to the chunk size, chunk size (16, or 4 for the stem)
  int tiles_x, tiles_y, cout_tiles, ntiles;
  int q_slots;          // conv2d_hs3x3q only: workgroups per XCD; each walks its XCD's units (hs3x3q_walk) in steps of q_slots
  int PH, PW, PWp;      // staged patch rows, columns, padded row pitch
  // conv2d_hs3x3 only: the input-channel chunks split over `ksplit` workgroups per tile (small batches: a 512->512 layer
  // on one 8x29 map is 8 tiles); part kpart covers chunks [kpart * cper, (kpart + 1) * cper) and writes its raw sums to
  // part + kpart * part_stride in the layout of y; conv2d_split_reduce_kernel adds them up and applies BN / residual / ReLU
  int ksplit, cper;
  float* part;
  size_t part_stride;
  // stem kernels only: a band's 32-column tiles (pooled stem: a strip's bands) split into segments of stem_seg_tiles, one workgroup each (few images:
  // a band of one 256x900 frame is 15 tiles walked by ONE workgroup otherwise); 0 = the whole band
  int stem_seg_tiles, stem_nseg;
  // generic split kernel only: depth-to-space store.  The conv's output channels are four groups of d2s_cin channels, one per
  // parity class (py, px) of a map of d2s_h x d2s_w pixels; channel g * d2s_cin + ci at (oy, ox) is stored to (and its residual
  // read from) channel ci at (2 oy + py, 2 ox + px), g = 2 py + px.  0 = plain NCHW store.  This is how the data gradient of a
  // stride-2 3x3 conv runs as ONE stride-1 2x2 conv on the low-resolution gradient (conv2d_hs_dgrad_s2).
  int d2s_cin, d2s_h, d2s_w;
  // conv2d_hs3x3 only (training forward): per-workgroup sums of the output and of its squares, [Cout][2][stats_p] floats
  // (p = (image, row tile, column tile)), pixels outside the map excluded; bn statistics then need no pass over the output
  float* stats_part;
  int stats_p;
  // conv2d_hs3x3 only (training backward, bs_raw != null): this launch is a data gradient whose output dx is the incoming
  // gradient of a BatchNorm (the conv BEFORE it in forward order).  Its epilogue then also leaves, in stats_part, that
  // BatchNorm's backward sums -- per channel the sum of dz and of dz * xhat over the workgroup's pixels, dz = dx * ReLU mask,
  // xhat = (raw - mean) * rstd -- so that no pass over dx has to compute them (channel_sums_kernel<1>).  bs_mask: 1 the
  // mask is `bs_out > 0` (ReLU after the residual add), 2 it is re-derived from the conv output: fma(raw, gamma rstd, beta -
  // mean gamma rstd) > 0 (ReLU straight after BatchNorm).
  const float* bs_raw; const float* bs_out; const float* bs_mean; const float* bs_rstd; const float* bs_gamma; const float* bs_beta;
  int bs_mask;
  // bs_mask == 1 with bs_bits != null: the mask as the forward pass left it (resnet_train.hip: bn_apply_groups_kernel), one BIT per
  // element -- byte [n][c / 8][pixel], bit c % 8 -- instead of the fp32 map bs_out
  const uint8_t* bs_bits;
  // bs_raw != null only: the residual `res` passes through a ReLU mask given as bits in the same layout (the identity path of a
  // BasicBlock's backward: res = d(block output), the mask = where the block's output was positive), so that the masked gradient
  // is never written as a tensor of its own
  const uint8_t* res_bits;
  // conv2d_hs3x3 only (inference executor): x / y / res in the cell layout instead of fp32 NCHW (conv2d_hs.hip: XCELLS)
  int x_cells, y_cells, res_cells;
  int vw;       // y_cells: columns of one image in the virtual row the column tiles run over (W + 1: the images side by side with
                // one shared all-zero column between neighbours; W for a single image)
  float inv_vw; // 1 / vw
  // inference executor only: the status word of the launch's layer group (adx_common.h: range_flag), or null
  uint32_t* status = nullptr;
};

// activation formats of one launch of the inference executor (bits)
constexpr int kFmtXCells = 1, kFmtYCells = 2, kFmtResCells = 4;
constexpr int kFmtXScaled = 8;      // with kFmtXCells: a data-gradient launch whose cell-layout x carries its scale (x_amax_n < 0)


}  // namespace adx

struct adx_resnet {
  int out_dim = 0;
  std::vector<adx::ConvSpec> convs;      // execution order: stem, then per block conv1, conv2, [downsample]
  std::vector<int> block_has_ds;         // per BasicBlock
  int t_fcw = 0, t_fcb = 0, n_tensors = 0;
  size_t o_fcw = 0, o_fcb = 0, packed_floats = 0;
  bool packed_once = false;
  // side streams of the inference executor (conv2d.hip: sub-batches of a large batch run on streams of their own so that one
  // sub-batch's launches fill the CUs another's last round of workgroups leaves idle); created on first use, per device
  static constexpr int kMaxSub = 4;
  hipStream_t side[kMaxSub - 1] = {nullptr, nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[kMaxSub - 1] = {nullptr, nullptr, nullptr};
  int side_device = -1;
  // range status (include/adx.h: adx_resnet_set_status): nblocks + 3 caller-owned device words, or null --
  // [0] stem (+ pool), [1 + b] BasicBlock b, [1 + nblocks] fc, [2 + nblocks] the weight images of adx_resnet_pack
  uint32_t* status = nullptr;
};

namespace adx {

// one conv2d launch: y = [relu](conv(x, w) [* scale + shift] [+ res]); w = packed [tap][cin_pad][cout]
// x_amax (optional, device): x_amax_n bit patterns whose maximum is max|x| over the whole input; the split-fp16 kernels use it to move x
// into fp16's normal range by an exact power of two (data gradients are far below 2^-14)
// stats_part (optional, stats_floats floats): where the launch may leave per-workgroup partial sums of its output and of its
// squares ([Cout][2][P] floats); *stats_p = P when it did (the pipelined 3x3 stride-1 kernel does), 0 when the caller has to
// compute the statistics from the output itself
struct BnBwdStats { const float* raw; const float* out; const float* mean; const float* rstd; const float* gamma; const float* beta; int mask;
                    const uint8_t* bits = nullptr; const uint8_t* res_bits = nullptr; };
int conv2d_launch_raw(const ConvSpec& L, const float* x, const float* w, const float* scale, const float* shift,
                      const float* res, float* y, int N, int H, int W, int relu, hipStream_t s,
                      const uint32_t* x_amax = nullptr, int x_amax_n = 0, float* stats_part = nullptr, size_t stats_floats = 0,
                      int* stats_p = nullptr, int fmt = 0, const BnBwdStats* bst = nullptr);

// ---- the plan of a 3x3 stride-1 split-fp16 launch ----
// Which kernel serves such a launch, in which variant, on which grid and with how many statistics tiles is decided ONCE, by
// conv2d_hs3x3_plan: a pure function (no HIP call, no state) of what is known before the launch.  conv2d_launch_raw computes
// the plan and the launchers only carry it out; the executors ask the same function ahead of time which layouts a launch
// will take (the predicates below), so an answer cannot differ from what the launch then does.
enum { kHsNone = 0, kHs3x3 = 1, kHs3x3q = 2 };               // family: another kernel / conv2d_hs3x3_kernel / conv2d_hs3x3q_kernel
enum { kXScaleNone = 0, kXScaleDynamic = 1, kXScalePre = 2 }; // x_amax: none / partial maxima of |x| / the scale x was written under
struct Hs3x3Query {
  int N = 0, H = 0, W = 0;
  int fmt = 0;                    // kFmt* bits as the caller passes them
  size_t stats_floats = 0;        // floats of the statistics buffer on offer (0: none)
  int bst_mask = 0;               // BatchNorm-backward request (BnBwdStats::mask), 0: none
  bool bst_bits = false;          // ... with the mask as bits
  int x_scale = kXScaleNone;
  bool affine = false, relu = false, has_res = false;
  bool y_aligned = true, res_aligned = true;       // 16-byte alignment (the split reduction's vector accesses)
  size_t split_floats = 0;        // capacity of the split-reduction scratch (0: none)
  int cus = 0;                    // compute units the launch may use (launch_cus; sizes the persistent grid only)
};
struct Hs3x3Plan {
  bool admitted = false;          // the operand formats of the query are ones the launch can take (fmt == 0 always is)
  int family = kHsNone;
  int mode = 0;                   // tile mode 0 / 1 / 2 of conv2d_hs3x3_kernel
  int stats = 0;                  // STATS / TRAIN: 0 none, 1 output sums, 2 the consumer BatchNorm's backward sums
  bool xcells = false, ycells = false, vr = false;
  bool dma = false;               // conv2d_hs3x3q_kernel: LDS-DMA staging
  int ksplit = 1, cper = 0;
  int tiles_x = 0, tiles_y = 0, cout_tiles = 0, vw = 0, q_slots = 0;
  size_t grid = 0;
  int threads = 0;
  size_t lds = 0;
  int stats_tiles = 0;            // partial-sum slots per channel when stats != 0
  size_t stats_need = 0;          // floats those take: the sums and (data gradient) max |dz| per 64-channel slab
  bool pair = false;              // conv2d_hs3x3_kernel's PAIR form (16x16x32 MFMAs over two taps x 16 channels): a rule on the shape
                                  // and the switches only, never on the operand formats -- every format of a launch sums in one order
};
// ---- the stage table of conv2d_hs3x3_kernel's PAIR form (conv2d_hs.hip) ----
// K = 32 of a 16x16x32 MFMA = two taps x the 16 channels of a chunk.  A pair of chunks (e, o) -- e staged in patch copy E = 0, o
// in copy O = 1 -- is nine stages of two taps with one kernel column kw = stage % 3.  Copy E is read by stages 0-5 and copy O by
// stages 3-8, so chunk o lands in O during stages 0-2 of its own pair and the next pair's e in E during stages 6-8, one patch
// round per stage.  The kernel's stage loop and the export (adx_conv2d_hs3x3_pair_walk) both read this table.
struct HsPairTap { int odd, kh; };      // chunk of the pair (0: e, 1: o) = the patch copy read; kernel row
struct HsPairStage {
  HsPairTap tap[2];
  int pround;           // patch round written to LDS during this stage (fetched one stage earlier); -1: none
  int pnext;            // ... a round of 0: this pair's chunk o (copy O), 1: the next pair's chunk e (copy E)
};
__host__ __device__ constexpr HsPairStage hs_pair_stage(int i) {
  return i < 3 ? HsPairStage{{{0, 0}, {0, 1}}, i, 0} : (i < 6 ? HsPairStage{{{0, 2}, {1, 0}}, -1, 0} : HsPairStage{{{1, 1}, {1, 2}}, i - 6, 1});
}
// first cell of the weight run of tap slot t of stage i of chunk pair `pair`, from the image of the (64-channel slab, chunk 0)
__host__ __device__ constexpr int hs_pair_run(int pair, int i, int t) {
  return ((2 * pair + hs_pair_stage(i).tap[t].odd) * 9 + hs_pair_stage(i).tap[t].kh * 3 + i % 3) * 256;
}
Hs3x3Plan conv2d_hs3x3_plan(const ConvSpec& L, const Hs3x3Query& q, const DebugSwitches& sw = debug_switches());
// ---- the unit walk of conv2d_hs3x3q_kernel (conv2d_hs16.hip) ----
// A launch's work is `units` = spatial tiles x cout tiles pieces, unit u = spatial tile * cout_tiles + cout tile.  XCD x (workgroup
// b runs on XCD b & 7) owns the contiguous range [x units / 8, (x + 1) units / 8); workgroup (x, slot = b >> 3) visits first,
// first + Q, ... below end, Q = grid / 8 workgroups per XCD.  The kernel and the export (adx_conv2d_hs3x3q_walk) share the range
// (hs3x3q_walk) and the split of a unit (hs3x3q_unit); the loop `u += Q while u < end` is written in each.
struct HsQWalk { int first, end; };
__host__ __device__ inline HsQWalk hs3x3q_walk(int xcd, int slot, int units) {
  return HsQWalk{(int)(((long)xcd * units) >> 3) + slot, (int)(((long)(xcd + 1) * units) >> 3)};
}
struct HsQUnit { int sp, ct; };
__host__ __device__ inline HsQUnit hs3x3q_unit(int u, int cout_tiles) {
  const int sp = u / cout_tiles;
  return HsQUnit{sp, u - sp * cout_tiles};
}
// workgroups per XCD of such a launch: one unit per workgroup (the longest range), or as many as `cus` compute units hold
inline int hs3x3q_slots(int units, int cus, bool persistent) {
  const int longest = (units + 7) / 8;
  return persistent ? std::min(longest, std::max(1, cus / 8)) : longest;
}
// true when this launch will run the pipelined 3x3 stride-1 kernel as ONE launch (no split reduction): the launches whose
// input / output / residual may be in the cell layout (fmt: kFmt*)
inline bool conv2d_hs3x3_plain(const ConvSpec& L, int N, int H, int W) {
  Hs3x3Query q;
  q.N = N; q.H = H; q.W = W; q.fmt = kFmtXCells | kFmtYCells;
  return conv2d_hs3x3_plan(L, q).admitted;
}
// true when a training-forward launch of this conv (statistics in the epilogue, fp32 output) can read its input as a cell tensor
// (fmt = kFmtXCells together with stats_part): a 3x3 stride-1 split-fp16 launch with room for its partial sums in stats_floats
inline bool conv2d_hs3x3_train_cells(const ConvSpec& L, int N, int H, int W, size_t stats_floats) {
  Hs3x3Query q;
  q.N = N; q.H = H; q.W = W; q.fmt = kFmtXCells; q.stats_floats = stats_floats;
  return stats_floats > 0 && conv2d_hs3x3_plan(L, q).admitted;
}
// true when a data-gradient launch of this (dgrad) spec can read a cell-layout, pre-scaled gradient (fmt = kFmtXCells | kFmtXScaled)
inline bool conv2d_hs3x3_dgrad_cells(const ConvSpec& L, int N, int H, int W) {
  Hs3x3Query q;
  q.N = N; q.H = H; q.W = W; q.fmt = kFmtXCells | kFmtXScaled; q.x_scale = kXScalePre;
  return L.dgrad && conv2d_hs3x3_plan(L, q).admitted;
}
// true when a data-gradient launch of this spec (dx accumulated in place) with a BnBwdStats request of this mask form will run
// the statistics epilogue (the launches that can take BnBwdStats::res_bits)
inline bool conv2d_hs3x3_dgrad_stats(const ConvSpec& L, int N, int H, int W, bool x_cells, int bst_mask, bool bst_bits, size_t stats_floats) {
  Hs3x3Query q;
  q.N = N; q.H = H; q.W = W; q.stats_floats = stats_floats; q.bst_mask = bst_mask; q.bst_bits = bst_bits; q.has_res = true;
  q.fmt = x_cells ? kFmtXCells | kFmtXScaled : 0;
  q.x_scale = x_cells ? kXScalePre : kXScaleDynamic;
  const Hs3x3Plan p = conv2d_hs3x3_plan(L, q);
  return L.dgrad && p.admitted && p.stats == 2;
}
// [Cout][Cin][k][k] -> [tap][cin_pad][Cout]; dgrad = 1 packs the data-gradient view instead:
// [tap'][cout_pad as K][Cin as N] with the taps flipped (conv of dy with this image gives dx)
int conv2d_pack_raw(const float* w, float* packed, int cout, int cin, int k, int cin_pad, int dgrad, hipStream_t s);
// fp32 weights -> the layout the kernel chosen for `consumer` reads (fp32 [tap][cin_pad][cout], or the fp16 hi/lo
// split image of conv2d_hs.hip).  dgrad = 1: `w` is the forward weight [consumer.cin][consumer.cout][k][k] and the
// image is its data-gradient view (roles swapped, taps flipped).
int conv2d_pack_spec(const ConvSpec& consumer, const float* w, float* packed, int dgrad, hipStream_t s);
// conv2d_hs.hip: fp32-equivalent convolution on the fp16 matrix cores (hi/lo split operands, 3 MFMAs per product)
bool conv2d_hs_eligible(const ConvSpec& L, const DebugSwitches& sw = debug_switches());
// floats a layer's packed weight image takes (direct image, plus the Winograd F(2,3) image where that path applies)
size_t conv2d_packed_floats(const ConvSpec& L);
int conv2d_hs_pack(const ConvSpec& consumer, const float* w, void* packed, int dgrad, hipStream_t s);
// several split-fp16 weight images in one launch (not the stem's): cout / cin as conv2d_hs_pack takes them from a ConvSpec
// (dgrad = 1: the spec of the data-gradient conv, i.e. cout = the forward cin and cin_pad = cin = the forward cout)
struct HsPackJob { const float* w; void* packed; int cout, cin_pad, cin, taps, dgrad; };
bool conv2d_hs_pack_batchable(const ConvSpec& consumer, int dgrad);
int conv2d_hs_pack_many(const HsPackJob* jobs, int n, hipStream_t s);
// plan: of a 3x3 stride-1 launch (conv2d_launch_raw), null for every other
int conv2d_hs_launch(const ConvSpec& L, Conv2dArgs a, hipStream_t s, const Hs3x3Plan* plan = nullptr);
// conv2d_hs16.hip: the same convolution on v_mfma_f32_16x16x32_f16 where the plan picks it (same packed weights, same cell tensors;
// ADX_HS_MODE=0|1|2 keeps every launch on the 32x32x16 kernel)
int conv2d_hs3x3q_launch(const Hs3x3Plan& p, Conv2dArgs a, hipStream_t s);
// Data gradient of a 3x3 stride-2 pad-1 conv (forward weight w [cout][cin][3][3], forward input h x w, output oh x ow):
// dx [n][cin][h][w] (+= when accumulate) from dy [n][cout][oh][ow].  An input pixel of parity class (py, px) receives from
// 1 / 2 / 2 / 4 of the nine taps, and all of them lie in the 2x2 window [oy, oy+1] x [ox, ox+1] of dy with oy = iy >> 1,
// ox = ix >> 1: one stride-1 2x2 conv with 4 cin output channels and a depth-to-space store -- 16 tap-products per four
// pixels where convolving a zero-dilated gradient with the flipped 3x3 kernel spends 36.  wbuild (16 cout cin floats) and
// wimg (16 cout cin floats) are scratch.  Returns ADX_ERR_INVALID when the shape is outside the kernel's rules.
bool conv2d_hs_dgrad_s2_eligible(int cin, int cout);
int conv2d_hs_dgrad_s2(const float* w, const float* dy, float* dx, int accumulate, int N, int cin, int cout, int H, int W,
                       float* wbuild, float* wimg, const uint32_t* dy_amax, int dy_amax_n, hipStream_t s);
// scratch for split reductions of the launches issued by this thread until it is cleared (a region of the calling
// executor's workspace, consumed in stream order)
void conv2d_set_split_scratch(float* p, size_t floats);
// the status word (include/adx.h: adx_resnet_set_status) the split-fp16 launches and weight packs issued by this thread set
// until it is cleared (null: none); the inference executor points it at the word of the layer group it is issuing
void conv2d_set_status(uint32_t* word);
uint32_t* conv2d_status();
// stem conv + BN + ReLU + MaxPool2d(3, 2, 1) in one pass: writes only the pooled map [N][64][PH][PW]
int conv2d_hs_stem_pool(const ConvSpec& L, const float* x, const float* w, const float* scale, const float* shift,
                        float* pooled, int N, int H, int W, hipStream_t s, const uint8_t* frames_u8 = nullptr,
                        const float* mean = nullptr, const float* stdv = nullptr, int y_cells = 0);      // y_cells: pooled as a cell tensor
// conv1 (3x3 stride 2, +BN+ReLU) and the block's downsample (1x1 stride 2, +BN) in one pass over x; both must be
// conv2d_hs_eligible (the downsample's weights packed with conv2d_hs_pack_ds)
// scale / shift pairs may be null (identity: the training forward wants both raw conv outputs); relu applies to conv1 only
int conv2d_hs_launch_block_s2(const ConvSpec& c1, const ConvSpec& ds, const float* x, const float* w1, const float* scale1,
                              const float* shift1, float* y1, const float* wd, const float* scaled, const float* shiftd,
                              float* yd, int N, int H, int W, hipStream_t s, int x_cells = 0, int y_cells = 0, int relu = 1,   // x / both outputs in the cell layout
                              bool force_32 = false);     // keep the launch on conv2d_hs_kernel whatever the plan says (tests)
// ---- the plan of a fused block-entry launch ----
// conv2d_hs_launch_block_s2 runs conv2d_hs3x3q_s2_kernel (conv2d_hs16.hip: the 16x16x32 tile walk over parity planes) where this
// pure function says so, and conv2d_hs_kernel (32x32x16, one tile per workgroup) everywhere else.  Like conv2d_hs3x3_plan it sees
// only the layer's shape, the operand formats the caller chose and the switches -- never the stream or the call's history.
struct HsS2Query {
  int N = 0, H = 0, W = 0;        // the INPUT's size
  bool x_cells = false, y_cells = false;
  int cus = 0;                    // compute units the launch may use (launch_cus; sizes the persistent grid only)
};
struct HsS2Plan {
  bool q = false;                 // conv2d_hs3x3q_s2_kernel serves the launch
  int tiles_x = 0, tiles_y = 0, cout_tiles = 0, vw = 0, q_slots = 0;
  size_t grid = 0;
  int threads = 0;
  size_t lds = 0;
};
HsS2Plan conv2d_hs_s2_plan(const ConvSpec& c1, const ConvSpec& ds, const HsS2Query& q, const DebugSwitches& sw = debug_switches());
int conv2d_hs3x3q_s2_launch(const HsS2Plan& p, Conv2dArgs a, hipStream_t s);
// compute units of the calling thread's current device (conv2d.hip)
int device_cus(int* cus);
// ... that a conv2d_hs3x3q launch issued by this thread may use: the device's less the reserve -- the executor's while one is set
// (conv2d_set_reserve_cus; -1 clears it), ADX_HS_RESERVE_CUS otherwise -- a multiple of 8, at least 8, at most ADX_HS_GRID_CAP
int launch_cus(int* cus);
void conv2d_set_reserve_cus(int reserve);
inline int hs_usable_cus(int device, int reserve, int cap) {
  int n = std::max(8, (device - std::max(0, reserve)) & ~7);
  if (cap > 0) n = std::min(n, std::max(8, cap & ~7));
  return n;
}
// conv1 3x3 stride 2 on the split-fp16 kernel + a 1x1 stride-2 downsample of the same shape: one fused launch (conv2d.hip)
inline bool resnet_fuses_ds(const ConvSpec& c1, const ConvSpec& ds, const DebugSwitches& sw = debug_switches()) {
  return conv2d_hs_eligible(c1, sw) && c1.k == 3 && c1.stride == 2 && c1.pad == 1 && ds.k == 1 && ds.stride == 2 && ds.pad == 0 &&
         ds.cin == c1.cin && ds.cout == c1.cout;
}
// conv2d_wgrad_hs.hip: weight gradient of the 3x3 convs on the fp16 matrix cores; dw must be zero on entry
bool conv2d_wgrad_hs_eligible(int Cin, int Cout, int k, int stride, int pad);
// x_cells: x is a cell tensor (the layout of the inference executor's activations; resnet_train.hip keeps a block's first
// activation that way)
int conv2d_wgrad_hs(const float* x, const float* dy, float* dw, int N, int Cin, int H, int W, int Cout, int stride,
                    const uint32_t* dy_amax, int dy_amax_n, hipStream_t s, bool x_cells = false, bool dy_cells = false);
// ADX_WGRAD_DETERMINISTIC=1: scratch for the per-split copies of dw that conv2d_wgrad_hs reduces in index order (lent by the calling
// thread's executor until cleared; conv2d_wgrad_partials_floats() = what to lend, 0 when the switch is off)
void conv2d_wgrad_set_partials(float* p, size_t floats);
size_t conv2d_wgrad_partials_floats();
// conv2d_wgrad_stem_hs.hip: the stem's (7x7 stride 2, 3 -> 64) weight gradient on the fp16 matrix cores; dw must be zero on entry
bool conv2d_wgrad_stem_hs_eligible(int Cin, int Cout, int k, int stride, int pad);
int conv2d_wgrad_stem_hs(const float* x, const float* dy, float* dw, int N, int H, int W, const uint32_t* dy_amax, int dy_amax_n,
                         hipStream_t s);
inline int conv_out_dim(int h, int k, int s, int p) { return (h + 2 * p - k) / s + 1; }
inline size_t al64(size_t v) { return (v + 63) / 64 * 64; }

// ---- the plan of one eval forward (conv2d.hip) ----
// Everything adx_resnet_forward decides above the single launch -- sub-batches and the whole-batch prefix, the activation
// format of every edge, the buffer of every tensor, the scratch slice and the status group of every launch -- is decided ONCE, by
// resnet_eval_plan: a pure function (no HIP call, no state, no heap) of the network, the call's shape and the switches.  The
// executor only carries the plan out; adx_resnet_plan_describe (include/adx.h) exports it, one record per launch.
//
// The format rule.  An edge is a CELL tensor iff its producer can write cells and every reader reads cells.  With plain(c) =
// conv2d_hs3x3_plain(c, nf, H, W) at the conv's own map size and nf the segment's batch:
//   * a block READS cells iff it is a fused entry (resnet_fuses_ds(c1, ds)), or has no downsample and c1.stride == 1 &&
//     plain(c1) && plain(c2): conv1 reads the input, conv2 reads it again as the residual;
//   * the map between a block's convs is cells iff plain(c2) (fused entry; the downsample's output goes with it) or the block
//     has no downsample and reads cells;
//   * a block's output is cells iff plain(c2) && (it is the last block -- the average pool reads both -- || the next block reads cells);
//   * the pooled map is cells iff the fused stem + pool launch writes it and block 0 reads cells.
// At the hand-off from the whole-batch prefix (nf = batch) to a sub-batch (nf = its own size) the producer's decision stands.
struct ResnetEvalQuery {
  int batch = 0, h = 0, w = 0;
  bool capturing = false;         // the caller's stream is being captured: one chain (no side streams)
  bool u8 = false;                // uint8 frames: the front-end lives in the fused stem + pool launch alone
};
// the workspace in floats: the stem region (the unpooled stem map, or split-reduction scratch where it is never written), then
// three rotating activation regions sized for the pooled map
struct ResnetLayout {
  int h1 = 0, w1 = 0, h2 = 0, w2 = 0;       // stem map, pooled map
  size_t stem = 0, act = 0;
  size_t floats() const { return stem + 3 * act; }
};
ResnetLayout resnet_layout(int batch, int h, int w);
constexpr int kResnetMaxBlocks = 16;        // ResNet-34
constexpr int kResnetBufStem = 3;           // buffer indices: 0..2 the rotating regions, 3 the stem region, -1 none
struct ResnetBlockStep {
  int block = 0, c1 = 0;                    // the block, and its conv1 in adx_resnet::convs (conv2 and the downsample follow it)
  int H = 0, W = 0, OH = 0, OW = 0;         // the input map and the block's own
  bool fused_ds = false;                    // conv1 + downsample as one block-entry launch
  int in = 0, mid = 0, id = 0, out = 0;     // buffers of the input, conv1's output, the identity (= in without a downsample), the output
  bool in_cells = false, mid_cells = false, id_cells = false, out_cells = false;
  int status = 0;                           // status group (adx_resnet_status_name)
};
struct ResnetSegment {                      // the whole-batch prefix, or one sub-batch
  int id = 0;                               // 0: the prefix, 1 + k: sub-batch k
  int n0 = 0, n = 0, nf = 0;                // images [n0, n0 + n); nf: the batch its format decisions are made for
  int stream = 0;                           // 0: the caller's, k: side stream k - 1
  size_t scratch_off = 0, scratch_floats = 0;   // its slice of the stem region as split-reduction scratch (0, 0 where the region is written)
  bool stem = false, stem_fused = false, pooled_cells = false;
  int nsteps = 0;
  ResnetBlockStep steps[kResnetMaxBlocks];
  int final_buf = 0, final_h = 0, final_w = 0;  // what the average pool reads (sub-batches only)
  bool final_cells = false;
};
struct ResnetEvalPlan {
  int nsub = 1, first_split = 0;            // blocks [0, first_split) run once, on the whole batch (with the stem when first_split > 0)
  int reserve_cus = 0;                      // compute units the pass's persistent conv2d_hs3x3q launches leave free (chosen with nsub)
  ResnetLayout lay;
  int nseg = 0;                             // (first_split > 0) + nsub: the prefix first
  ResnetSegment seg[1 + adx_resnet::kMaxSub];
};
// the reserve of a pass that keeps one chain as today (small batches, captures, ADX_CHECK_RANGE=1) / of an eval pass of B >= 32
// outside a capture: what the measurement of the four candidates chose (profiles/README.md, "The unit walk")
constexpr int kEvalReserveCus[2] = {0, 0};
// ADX_ERR_INVALID (with the message set) for a shape or format hand-off the executor cannot run
int resnet_eval_plan(const adx_resnet& r, const ResnetEvalQuery& q, ResnetEvalPlan* plan, const DebugSwitches& sw = debug_switches());
// ADX_CHECK_RANGE=1 (no-op otherwise): fails with ADX_ERR_RANGE naming (what, index) when the tensor holds |x| >= 65504 or a
// non-finite value (cells: an fp16 hi half that is inf / NaN); synchronises the stream
int conv2d_range_check(const char* what, int index, const float* t, size_t floats, bool cells, hipStream_t s);
int maxpool_launch(const float* x, float* y, int planes, int H, int W, int OH, int OW, hipStream_t s);
int avgpool_fc_launch(const float* x, const float* fw, const float* fb, float* out, int batch, int C, int HW, int out_dim,
                      hipStream_t s, int x_cells = 0, uint32_t* status = nullptr);

}  // namespace adx
