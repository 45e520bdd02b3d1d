/*
 * adx.h — C ABI of libadx.so, the MI355X (gfx950) implementation of the diffusion
 * trajectory-denoising hot path of Justin900429/autonomous_driving_with_diffusion_model.
 *
 * The reference has no FFI layer: its boundary is the Python call surface
 * (SURVEY.md §8b).  This header is the boundary one level below it: every entry point
 * takes raw device pointers, plain sizes and a hipStream_t (passed as void*), returns an
 * int status (0 = ok, <0 = error; adx_last_error() gives the message) and never allocates
 * device memory — workspaces are sized by *_bytes() queries and owned by the caller.
 * All tensors are fp32, contiguous row-major unless a stride is given; integer schedule
 * indices are int64.  Each entry cites the reference code it replaces
 * (paths relative to the reference checkout).
 */
#ifndef ADX_H
#define ADX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADX_OK 0
#define ADX_ERR_INVALID (-1)   /* bad argument / unsupported shape */
#define ADX_ERR_HIP (-2)       /* a HIP runtime call failed */
#define ADX_ERR_STATE (-3)     /* object used before it was initialised */
#define ADX_ERR_RANGE (-4)     /* ADX_CHECK_RANGE=1 only: an activation left the fp16 range of the split kernels */

typedef void* adx_stream;      /* hipStream_t */

int adx_version(void);
/* sha256 (first 32 hex digits) of the sources this library was built from (csrc/build.sh); "unknown" for ad-hoc builds */
const char* adx_source_hash(void);
const char* adx_last_error(void);

/* ------------------------------------------------------------------------------------
 * Temporal stack, op level (each op is one kernel launch).
 * -----------------------------------------------------------------------------------*/

/* Geometry of one temporal convolution, y = epilogue(conv(x)).
 *   kind 0: Conv1d(k=taps, stride, padding=pad)           modeling/helpers.py:80,104; temporal.py:40-44,192
 *   kind 1: ConvTranspose1d(k=taps, stride=2, padding=1)  modeling/helpers.py:89
 * The input may be the channel-concatenation of two tensors (skip connection,
 * modeling/temporal.py:227): channels [0,c0) come from x0, [c0,c0+c1) from x1.
 * Strides are in elements so that [B,H,D] trajectories can be read/written in place
 * (the einops rearranges at modeling/temporal.py:204,243).                              */
typedef struct adx_tconv_desc {
  int32_t kind, taps, stride, pad;
  int32_t c0, c1, cout;
  int32_t lin, lout;
  int32_t groups;            /* 0: no GroupNorm/Mish epilogue; 8: Conv1dBlock (helpers.py:95-112) */
  float eps;
  /* weight source layout for adx_tconv_pack (0,0 = the module's own weight).  The data-gradient of a
   * convolution is again a convolution of this family with the SAME weight tensor read differently:
   *   w_layout 0: w[cout][cin][taps]   1: w[cin][cout][taps];   w_flip 1: taps reversed.          */
  int32_t w_layout, w_flip;
  /* 0 (default): split-fp16 MFMA where the geometry allows it (fp32-grade result, csrc/tconv_hs.hip);
   * 1: the exact-fp32 MFMA kernel (used for gradient-sized operands whose range fp16 cannot hold). */
  int32_t exact;
  /* Lengths that are not powers of two (the reference accepts any horizon divisible by 8, modeling/temporal.py:59-75:
   * 24 -> 24, 12, 6, 3): `lin` / `lout` are then the lengths rounded up to powers of two (the kernels' index arithmetic)
   * and these the real ones; positions >= lin_valid read as zero, positions >= lout_valid are neither stored nor counted
   * in the GroupNorm statistics.  0 = equal to lin / lout.  Such descriptors run on the exact-fp32 kernel; adx_tconv_wgrad
   * honours the same fields, and the training executor passes them to every backward kernel. */
  int32_t lin_valid, lout_valid;
} adx_tconv_desc;

/* Size (bytes) of the packed weight image for a conv of this geometry. */
size_t adx_tconv_packed_bytes(const adx_tconv_desc* d);

/* Pack a PyTorch-layout weight ([cout][cin][taps] for kind 0, [cin][cout][taps] for kind 1)
 * into the MFMA B-operand fragment order read by adx_tconv_forward. */
int adx_tconv_pack(const adx_tconv_desc* d, const float* w, float* packed, adx_stream s);

typedef struct adx_tconv_io {
  const float* x0; int64_t x0_sb, x0_sc, x0_sl;   /* input 0 and its batch/channel/position strides */
  const float* x1; int64_t x1_sb, x1_sc, x1_sl;   /* input 1 (NULL when c1 == 0) */
  const float* packed_w;                          /* from adx_tconv_pack */
  const float* bias;                              /* [cout] or NULL */
  const float* gamma; const float* beta;          /* GroupNorm affine [cout] (groups > 0) */
  const float* tbias; int64_t tbias_stride;       /* additive time bias [B][...] (temporal.py:53) or NULL */
  const float* res; int64_t res_sb, res_sc, res_sl; /* residual added last (temporal.py:55) or NULL */
  float* y; int64_t y_sb, y_sc, y_sl;
  int32_t batch;
  /* training only (NULL otherwise): conv+bias before GroupNorm, dense [B][cout][lout], and the
   * per-(sample, group) statistics [B][groups][2] = (mean, rstd) that the backward pass reuses */
  float* pre; float* stats;
  /* optional device scratch (scratch_floats floats, contents irrelevant): lets a launch whose grid would occupy a few CUs
   * only (tiny batches) split its reduction over more workgroups and finish with a reduce launch.  NULL: never split. */
  float* scratch; int64_t scratch_floats;
  /* optional (NULL: absent), with `scratch`: 256 device words that are ZERO when the call is enqueued.  A split reduction then
   * needs no reduce launch: the last workgroup to publish its partial tile adds them up and leaves the words zero again, so
   * the same words serve every later call on the same stream (one word per workgroup of the unsplit grid, which is at
   * most 128 for a launch that splits). */
  uint32_t* tickets;
} adx_tconv_io;

/* Conv (+bias) [-> GroupNorm -> Mish] [+ time bias] [+ residual], fp32 MFMA.
 * Replaces Conv1dBlock.forward / Downsample1d / Upsample1d / the 1x1 residual and head convs. */
int adx_tconv_forward(const adx_tconv_desc* d, const adx_tconv_io* io, adx_stream s);

/* SinusoidalPosEmb + time_mlp (+ cond_mlp) + cat(img_feature) + Mish:
 * modeling/helpers.py:62-74, modeling/temporal.py:88-98,205-213.
 * rows = effective batch; t has t_rows entries and img_feature feat_rows rows, both
 * broadcast by `r % n` exactly like the reference's .repeat (temporal.py:208-211).
 * Outputs: time_embed [rows][dim] (after the cond_mlp add) and
 *          mish_cond  [rows][2*dim] = Mish(cat(time_embed, img_feature)).               */
typedef struct adx_embed_weights {
  const float* freqs;                    /* [dim/2] host-computed exp(-i*ln(1e4)/(dim/2-1)) */
  const float* w1; const float* b1;      /* time_mlp.1: [4dim][dim] */
  const float* w3; const float* b3;      /* time_mlp.3: [dim][4dim] */
  const float* cw0; const float* cb0;    /* cond_mlp.0: [dim][2]   (NULL unless FREE_GUIDANCE) */
  const float* cw2; const float* cb2;    /* cond_mlp.2: [dim][dim] */
} adx_embed_weights;
int adx_embed_forward(const adx_embed_weights* w, int32_t dim, const int64_t* t, int32_t t_rows,
                      const float* cond /* [rows][2] or NULL (=> zeros) */,
                      const float* img_feature, int32_t feat_rows, int32_t rows,
                      float* time_embed, float* mish_cond, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Whole-UNet executor (one call = TemporalMapUnet.forward without the perception pass,
 * modeling/temporal.py:204-245).  Weights are handed over once in the reference's
 * parameter registration order and packed into a caller-owned buffer.
 * -----------------------------------------------------------------------------------*/
typedef struct adx_unet adx_unet;

typedef struct adx_unet_config {
  int32_t horizon, transition_dim, dim;
  int32_t n_mults; int32_t dim_mults[8];
  int32_t guidance;          /* 0 NO_GUIDANCE, 1 FREE_GUIDANCE, 2 CLASSIFIER_GUIDANCE (misc/constant.py:17-20) */
} adx_unet_config;

int adx_unet_create(const adx_unet_config* cfg, adx_unet** out);
/* adx_unet_create with option flags.  ADX_UNET_ATTENTION: MODEL.USE_ATTN, the LayerNorm + LinearAttention block
 * (modeling/helpers.py:120-175) after each down level's and up level's second residual block and between the mid blocks.
 * Accepted only with n_mults >= 2, all dim_mults equal and a horizon of at most 64: the reference builds the up levels'
 * attention for dim_out channels and applies it to dim_in (temporal.py:168,226-231), so its forward fails on every other
 * configuration.  Its parameters are registered as downs.{i}.2, mid_attn, ups.{i}.2: to_qkv.weight, to_out.weight,
 * to_out.bias, norm.g, norm.b. */
#define ADX_UNET_ATTENTION 1
int adx_unet_create_ex(const adx_unet_config* cfg, int32_t flags, adx_unet** out);
void adx_unet_destroy(adx_unet* u);
/* number of parameter tensors expected by adx_unet_pack (the non-perception parameters,
 * in named_parameters() order; TrajPredict's are accepted but handled by adx_trajpred_*) */
int adx_unet_num_params(const adx_unet* u);
/* Range status of the temporal stack, as adx_resnet_set_status for the perception pass: the split-fp16 temporal kernels
 * (modeling/temporal.py:204-244 and helpers.py's Conv1dBlock / ResidualTemporalBlock in the reference, fp32 there) OR a
 * nonzero value into the word of the layer group whose launch splits a value with |x| >= 65504 or a NaN -- in staging, or
 * where a chained / pipelined launch forms the next conv's input.  The value counts where it is split, i.e. at the conv that
 * reads it.  Groups: i "down<i>" (down level i; the trajectory x and the time bias count as down0), n "mid", n + 1 + i
 * "up<i>" (a chained last up level carries the head: its splits count there), 2n "head", 2n + 1 "weights" (the split weight
 * images of adx_unet_pack).  Written by adx_unet_forward, adx_unet_time_conditioning and adx_unet_pack, never by training. */
int32_t adx_unet_status_words(const adx_unet* u);
int adx_unet_set_status(adx_unet* u, uint32_t* words /* device, adx_unet_status_words(u) words, or NULL */);
const char* adx_unet_status_name(const adx_unet* u, int32_t group);
size_t adx_unet_packed_bytes(const adx_unet* u);
int adx_unet_pack(adx_unet* u, const float* const* params, int32_t n_params, const float* freqs,
                  void* packed, adx_stream s);
/* The workspace needs no initialisation.  Its first 256 words are the ticket words of adx_tconv_io::tickets (at a place
 * that does not depend on `rows`); adx_unet_forward clears them itself at the head of every call. */
size_t adx_unet_workspace_bytes(const adx_unet* u, int32_t rows);

typedef struct adx_unet_io {
  const float* x;             /* [rows][horizon][transition_dim] */
  const float* img_feature; int32_t feat_rows;   /* perception output [feat_rows][dim] */
  const int64_t* t; int32_t t_rows;
  const float* cond;          /* [rows][2] or NULL */
  int32_t rows;
  float* out;                 /* [rows][horizon][transition_dim] (NO/FREE) or action [rows][horizon][3] (CLASSIFIER) */
  float* time_embed;          /* [rows][dim] or NULL (CLASSIFIER: returned to the caller, temporal.py:236-237) */
  /* Optional (zero = absent), for sampling loops.
   * x_rows: rows of `x` actually present: `rows` (default) or 1 -- every row then reads the one trajectory, which is the
   *   classifier-free pair torch.cat([trajs, trajs]) of interact.py:131 at B = 1 without building it.
   * time_bias: this call's [rows][adx_unet_time_bias_width] slice of a table made by adx_unet_time_conditioning; t, cond
   *   and img_feature are then not read and time_embed must be NULL (the caller holds the table's time_embed). */
  int32_t x_rows;
  const float* time_bias;
} adx_unet_io;
int adx_unet_forward(adx_unet* u, const void* packed, void* workspace, const adx_unet_io* io, adx_stream s);
/* Everything of the forward that depends on (t, cond, img_feature) only -- the time MLP, the condition MLP and the
 * time_mlp Linear of all 16 residual blocks (modeling/temporal.py:206-216, modeling/helpers.py:121-123) -- for `rows`
 * rows at once, e.g. all 50 timesteps of a sampling loop x the rows of one step: inside the loop
 * (interact.py:128-166) these are the same launches every tick, and none of them depends on the trajectory.  Uses
 * io->t, t_rows, cond, img_feature, feat_rows, rows (workspace sized by adx_unet_time_conditioning_workspace_bytes(u,
 * rows): two small per-row vectors, not a forward's activation ring).  Writes
 * time_bias [rows][adx_unet_time_bias_width(u)] and, if not NULL, time_embed [rows][dim].  Row-wise identical to what
 * adx_unet_forward computes internally. */
int32_t adx_unet_time_bias_width(const adx_unet* u);
size_t adx_unet_time_conditioning_workspace_bytes(const adx_unet* u, int32_t rows);
int adx_unet_time_conditioning(adx_unet* u, const void* packed, void* workspace, const adx_unet_io* io, float* time_embed,
                               float* time_bias, adx_stream s);
/* For tests only: a read-only description of where a forward of `rows` rows keeps the hand-off state of the deepest level's
 * pipeline launch (csrc/tconv_pipe.hip) in the caller's workspace -- computed by the function the forward itself lays the
 * workspace out with.  Locations are BYTE OFFSETS into the workspace; -1 = the forward of `rows` rows has no such region.
 *   ints[8]  = {shape_ok, runs, C, L, P, n_tickets, epoch_slot, 0}
 *              shape_ok: the configuration and `rows` fit the pipeline launch (decided on the host);
 *              runs: a forward of this process on the current device takes it -- shape_ok, ADX_UNET_PIPE not 0, and the
 *              device's forward-number counter exists (made by the first adx_unet_pack on the device);
 *              C, L: channels and positions of the deepest level; P = C / 16 workgroups per stage;
 *              n_tickets (256) 32-bit ticket words at offs[0], of which word epoch_slot (240) holds the forward's number
 *   offs[12] = {tickets, scratch, scratch_bytes, ksplit_bytes, records, record_bytes, ya, yb, yc, y_bytes, workspace_bytes, 0}
 *              scratch: the split-reduction scratch, of which the first ksplit_bytes are handed to the K-split launches and
 *              the rest is the pipeline's alone; records: the seven stages' tagged 16-byte units {d0, d1, d2, tag};
 *              ya, yb, yc: the block outputs later stages of the same launch read, y_bytes each (records .. y_bytes: -1
 *              unless shape_ok); workspace_bytes = adx_unet_workspace_bytes(u, rows).
 * Refuses (ADX_ERR_*) a null handle or output and rows < 1. */
int adx_unet_pipe_describe(const adx_unet* u, int32_t rows, int32_t* ints, int64_t* offs);

/* For tests only: the launch plan of ONE eval forward of `rows` rows, one record per launch in launch order.  Needs no GPU,
 * launches nothing and allocates nothing on a device: the call runs the forward's own host code -- the tile, split, chain
 * and pipeline decisions of adx_unet_forward themselves, with the scratch and ticket words a forward owns -- on placeholder
 * addresses, with every launch function recording its finished argument block instead of launching (csrc/plan.h).  The
 * process-wide switches (ADX_UNET_CHAIN, ADX_UNET_PIPE, ADX_CHAIN_MASK, ADX_TCONV_EXACT) act as they do on a forward.
 * The forward planned passes every per-row input (x_rows = t_rows = feat_rows = rows; `cond` under FREE_GUIDANCE), or,
 * with ADX_PLAN_TIME_BIAS, a precomputed time_bias.  Whether the deepest level takes the pipeline launch also depends on
 * the process (adx_unet_pipe_describe: runs); ADX_PLAN_ASSUME_PACKED plans as in a process whose device has seen an
 * adx_unet_pack, which is how a CPU-only process learns what a GPU process launches.
 * ints: ADX_PLAN_INTS words per record, at most max_records records (more launches: ADX_ERR_INVALID); *n_records: launches.
 *   [0] group    layer group as the status words number them (adx_unet_status_name); a launch without weights counts with
 *                the launch before it
 *   [1] block    residual block within the group (0, 1), or -1
 *   [2] conv     ADX_PLAN_CONV_*: which conv of the block / group (LEVEL: a whole chained level; RUN: the pipeline's seven
 *                convs), or -1 for a launch without weights
 *   [3] family   ADX_PLAN_*: the kernel
 *   [4] bt, [5] row_tiles = ceil(rows / bt), [6] rows % bt: samples per row tile (the pipeline holds every row in one)
 *   [7] ctiles   workgroups along the output channels (pipeline: 7 stages x P + the finisher)
 *   [8] grid     = row_tiles x (ctiles x ksplit + ctiles_b)
 *   [9] ksplit   workgroups sharing one (row tile, channel tile)'s reduction; [10] reduce: 0 no split, 1 ticket words, 2 a
 *                reduce launch follows (its own record, family ADX_PLAN_REDUCE)
 *   [11] chunks  staged input chunks one workgroup walks = ceil(min(channels of its share, cin_pad) / ck)
 *   [12] vec_stage, [13] fast_epi, [14] live taps
 *   [15] block_b, [16] conv_b, [17] ctiles_b: the second conv of a pair / mixed launch (-1, -1, 0 otherwise)
 *   [18] ck, [19] cin_pad: channels per staged chunk, padded input channels
 *   [20] part_floats, [21] part_off: ksplit > 1: the partial tiles' footprint and where it starts, in floats from the start of
 *                the forward's split scratch (adx_unet_pipe_describe: offs[1]); -1: none
 *   [22] dynamic LDS bytes, [23] lout, [24] cout (of the launch's last conv), [25] which launch without weights (1 time / condition
 *                embedding, 2 ticket reset, 3 attention LayerNorm, 4 attention core), [26], [27] 0 */
#define ADX_PLAN_INTS 28
#define ADX_PLAN_ASSUME_PACKED 1
#define ADX_PLAN_TIME_BIAS 2
enum { ADX_PLAN_AUX = 0, ADX_PLAN_PIPE = 1, ADX_PLAN_CHAIN = 2, ADX_PLAN_KSPLIT = 3, ADX_PLAN_SHORTK = 4, ADX_PLAN_SHORTK_PAIR = 5,
       ADX_PLAN_MIXED = 6, ADX_PLAN_GENERIC = 7, ADX_PLAN_EXACT = 8, ADX_PLAN_REDUCE = 9 };
enum { ADX_PLAN_CONV_A = 0, ADX_PLAN_CONV_B = 1, ADX_PLAN_CONV_R = 2, ADX_PLAN_CONV_DOWN = 3, ADX_PLAN_CONV_UP = 4,
       ADX_PLAN_CONV_HEAD0 = 5, ADX_PLAN_CONV_HEAD1 = 6, ADX_PLAN_CONV_TLIN = 7, ADX_PLAN_CONV_QKV = 8, ADX_PLAN_CONV_ATTN_OUT = 9,
       ADX_PLAN_CONV_LEVEL = 10, ADX_PLAN_CONV_RUN = 11 };
int adx_unet_plan_describe(const adx_unet* u, int32_t rows, int32_t flags, int32_t* n_records, int32_t* ints, int32_t max_records);
/* The same for one adx_tconv_forward call on dense 16-byte aligned tensors of `batch` samples with a scratch of
 * scratch_floats floats (0: none) and, if has_tickets, ticket words: group 0, block -1, conv 0, part_off 0. */
int adx_tconv_plan_describe(const adx_tconv_desc* d, int32_t batch, int64_t scratch_floats, int32_t has_tickets, int32_t* n_records,
                            int32_t* ints, int32_t max_records);

/* ------------------------------------------------------------------------------------
 * Training step T1 (train.py:242-251), temporal stack: forward that keeps a tape, and backward.
 * The reference gets these from torch autograd; the gradients are written in PyTorch layouts.
 * -----------------------------------------------------------------------------------*/
typedef struct adx_unet_tape adx_unet_tape;
int adx_unet_tape_create(adx_unet_tape** out);
void adx_unet_tape_destroy(adx_unet_tape* t);
size_t adx_unet_train_workspace_bytes(const adx_unet* u, int32_t rows);
int adx_unet_forward_train(adx_unet* u, const void* packed, void* workspace, size_t workspace_bytes,
                           const adx_unet_io* io, adx_unet_tape* tape, adx_stream s);
/* d_out [rows][H][D] -> one gradient per parameter of adx_unet_pack's list (written) and
 * d_img_feature [rows][dim] (gradient entering the perception encoder).  `params` are the same
 * raw parameter pointers given to adx_unet_pack (the data-gradient convs re-read them). */
int adx_unet_backward(adx_unet* u, const void* packed, void* workspace, size_t workspace_bytes, adx_unet_tape* tape,
                      const float* d_out, const float* d_time_embed /* extra gradient into time_embed or NULL */,
                      float* d_img_feature, const float* const* params, float* const* grads, int32_t n_grads,
                      adx_stream s);
/* op level: gradient through [+tb] -> Mish -> GroupNorm of a Conv1dBlock (modeling/helpers.py:105-108) */
int adx_gn_mish_backward(const float* dy, int64_t dy_sb, int64_t dy_sc, int64_t dy_sl, const float* pre,
                         const float* stats, const float* gamma, const float* beta, float* dc, float* dgamma,
                         float* dbeta, float* dbias, float* dtb, int64_t dtb_stride, int32_t B, int32_t C, int32_t L,
                         int32_t groups, adx_stream s);
/* op level: dW[cout][cin][taps] of a (kind 0) temporal conv from its input (io->x0/x1) and d(conv out) */
int adx_tconv_wgrad(const adx_tconv_desc* d, const adx_tconv_io* io, const float* dc, float* dw, adx_stream s);
int adx_bias_grad(const float* dc, float* db, int32_t B, int32_t C, int32_t L, adx_stream s);
/* The same two ops with the arguments the training executor passes.  adx_gn_mish_backward_ex: L is the padded (power of
 * two) length, L_valid the real one (0: L): positions >= L_valid are not read, count in no sum, and come out zero in dc.
 * dgamma, dbeta, dbias (may be NULL) are added to (the caller zeroes them); dtb (may be NULL) is written where L <= 64 and
 * added to beyond.  adx_bias_grad_ex: db[c] = sum over b and l < L_valid of dc[b * sb + c * sc + l * sl] (written). */
int adx_gn_mish_backward_ex(const float* dy, int64_t dy_sb, int64_t dy_sc, int64_t dy_sl, const float* pre,
                            const float* stats, const float* gamma, const float* beta, float* dc, float* dgamma,
                            float* dbeta, float* dbias, float* dtb, int64_t dtb_stride, int32_t B, int32_t C, int32_t L,
                            int32_t groups, int32_t L_valid, adx_stream s);
int adx_bias_grad_ex(const float* dc, int64_t sb, int64_t sc, int64_t sl, float* db, int32_t B, int32_t C, int32_t L,
                     int32_t L_valid, adx_stream s);
/* For tests only: the launch geometry adx_tconv_wgrad (and the training executor) uses for `batch` samples -- the function
 * the launch itself calls; host arithmetic, needs no GPU.  ints: ADX_WGRAD_PLAN_INTS words
 *   [0] per4        samples per MFMA K-step of 4 (sample, position) rows: 1 for lout >= 4, else 4 / lout
 *   [1] nfo         16-channel output fragments per workgroup (4, 2 or 1)
 *   [2] n_ci_tiles  16-channel input tiles, [3] n_co_tiles: (16 nfo)-channel output tiles, [4] tiles = their product
 *   [5] nsplit      workgroups that share one weight tile (1: plain stores, more: float atomics onto the zeroed dW)
 *   [6] nb          samples per workgroup: split i reduces samples [i nb, min((i + 1) nb, batch))
 *   [7] sbt         samples per staged super-tile (the kernel walks its nb samples sbt at a time; sbt lout <= 128 rows)
 *   [8] pl, [9] lp  left zero pad and per-sample pitch of the staged input, [10] rs: LDS row stride = sbt lp + 1
 *   [11] staging bytes, [12] reduction bytes, [13] dynamic LDS bytes (their maximum)
 *   [14] grid = tiles nsplit, [15] 0 */
#define ADX_WGRAD_PLAN_INTS 16
int adx_tconv_wgrad_plan_describe(const adx_tconv_desc* d, int32_t batch, int32_t* ints);
/* op level, the attention block's own kernels (csrc/attn.hip); L is the padded length (<= 64 for the core), L_valid the
 * real one (0: L).  LayerNorm over channels of x [B][C][L] (strided) -> dense xn [B][C][L] and, when not NULL, the
 * per-(sample, position) mean and rstd [B][L] the backward needs. */
int adx_chan_layernorm_forward(const float* x, int64_t sb, int64_t sc, int64_t sl, const float* g, const float* b, float* xn,
                               float* mean, float* rstd, int32_t B, int32_t C, int32_t L, int32_t L_valid, adx_stream s);
/* dy dense [B][C][L] -> dx dense [B][C][L] (written, or added to with accumulate != 0), dg and db [C] (written) */
int adx_chan_layernorm_backward(const float* dy, const float* x, int64_t sb, int64_t sc, int64_t sl, const float* mean,
                                const float* rstd, const float* g, float* dx, float* dg, float* db, int32_t B, int32_t C,
                                int32_t L, int32_t L_valid, int32_t accumulate, adx_stream s);
/* qkv dense [B][384][L] (to_qkv's output) -> o dense [B][128][L]; the backward takes dO [B][128][L] -> dqkv [B][384][L] */
int adx_linattn_forward(const float* qkv, float* o, int32_t B, int32_t L, int32_t L_valid, adx_stream s);
int adx_linattn_backward(const float* qkv, const float* dout, float* dqkv, int32_t B, int32_t L, int32_t L_valid, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Perception: ResNet-34 forward (eval mode, BatchNorm folded at pack time),
 * modeling/resnet.py:56-102,163-296 with fc = Linear(512, dim) (temporal.py:83-84).
 * -----------------------------------------------------------------------------------*/
typedef struct adx_resnet adx_resnet;
int adx_resnet_create(int32_t out_dim, adx_resnet** out);
void adx_resnet_destroy(adx_resnet* r);
int adx_resnet_num_tensors(const adx_resnet* r);     /* state_dict entries excluding num_batches_tracked */
size_t adx_resnet_packed_bytes(const adx_resnet* r);
/* tensors: the perception.* state_dict entries in order, num_batches_tracked skipped
 * (conv weight, bn weight, bn bias, bn running_mean, bn running_var, ..., fc weight, fc bias) */
int adx_resnet_pack(adx_resnet* r, const float* const* tensors, int32_t n, void* packed, adx_stream s);
size_t adx_resnet_workspace_bytes(const adx_resnet* r, int32_t batch, int32_t h, int32_t w);
/* Stream semantics: everything the call enqueues is ordered behind `s`'s earlier work and in front of its later work.  At
 * batch >= 32 (outside a stream capture) the pass runs as two sub-batches: one on `s`, one on a side stream the HANDLE owns
 * (created on first use, destroyed with the handle; forked from `s` and joined into `s` by events inside the call) -- one
 * sub-batch's launches fill the CUs the other's last round of workgroups leaves idle.  Same kernels and per-image arithmetic;
 * ADX_RESNET_STREAMS=1 keeps one chain.  A handle must not be driven from two host threads at once. */
int adx_resnet_forward(adx_resnet* r, const void* packed, void* workspace, const float* img /* NCHW */,
                       int32_t batch, int32_t h, int32_t w, float* feature /* [batch][out_dim] */, adx_stream s);
/* The same with the agents' image front-end folded into the stem's staging load: frames_hwc = uint8 camera frames
 * [batch][h][w][3] (RGB); ToTensor + Normalize(mean, std) (interact.py:73-78, e2e_driving/diffusion_agent.py:96-101) are
 * applied on the fly -- (v / 255 - mean[c]) / std[c], the arithmetic of adx_image_normalize -- and the fp32 NCHW image
 * is never materialised.  Bit-identical to adx_image_normalize followed by adx_resnet_forward. */
int adx_resnet_forward_u8(adx_resnet* r, const void* packed, void* workspace, const uint8_t* frames_hwc,
                          const float* mean /* [3] */, const float* stdv /* [3] */, int32_t batch, int32_t h, int32_t w,
                          float* feature /* [batch][out_dim] */, adx_stream s);
/* Range status.  The split-fp16 kernels carry operands as x = hi + lo / 2^11 in fp16, so a value with |x| >= 65504 (or a
 * NaN) that one of them splits becomes inf / NaN and travels on silently, where the reference's fp32 forward
 * (modeling/resnet.py:87-102,163-296) stays finite.  With a status buffer attached, every launch of adx_resnet_forward /
 * adx_resnet_forward_u8 / adx_resnet_pack ORs a nonzero value into the uint32 word of its layer group when it splits or
 * stores such a value: no synchronisation, graph-capture safe, outputs bit-identical with and without the buffer.
 * The words are sticky: only the caller clears them (e.g. hipMemsetAsync).  Groups, in this order:
 *   0 "stem" (conv1 + bn1 + relu + maxpool; the input image's values count here), 1 + b "block<b>" (BasicBlock b, b < 16,
 *   the numbering of ADX_CHECK_RANGE's message), 17 "fc" (avgpool + fc), 18 "weights" (the split weight images of
 *   adx_resnet_pack).
 * adx_resnet_status_words(r) = the number of words (<0 on a null handle); adx_resnet_set_status(r, words) attaches a
 * device buffer of that many words (NULL detaches); adx_resnet_status_name(r, g) = group g's name (NULL on a bad index).
 * The training forward (adx_resnet_forward_train) never writes the words; ADX_CHECK_RANGE=1 is unchanged. */
/* For tests only: the plan of ONE eval forward of `batch` images of h x w, one record per launch in issue order.  Needs no
 * GPU and launches nothing: the call runs the pure function the executor itself carries out (csrc/conv2d_internal.h:
 * resnet_eval_plan), which decides the sub-batches, the activation format and buffer of every tensor, the scratch slice and
 * the status group of every launch.  Which kernel serves a launch, its tiles and its reduction split are decided below that,
 * per launch, and are not part of this export.  The process-wide switches (ADX_RESNET_STREAMS, ADX_RESNET_SPLIT_FROM,
 * ADX_CHECK_RANGE, ADX_CONV_EXACT, ADX_CONV_CELLS, ...) act as they do on a forward.
 * flags: ADX_RESNET_PLAN_CAPTURING plans the forward as inside a stream capture (one chain, no side streams).
 * ints: ADX_RESNET_PLAN_INTS words per record, at most max_records records (more launches: ADX_ERR_INVALID); *n_records: launches.
 *   [0] segment  0: the whole-batch prefix in front of the fork (the stem and blocks [0, first_split)), 1 + k: sub-batch k
 *   [1] stream   0: the caller's, k: side stream k - 1
 *   [2] n0, [3] n: the segment's images [n0, n0 + n); [4] nf: the batch its format decisions are made for
 *   [5] kind     ADX_RESNET_PLAN_*: stem + pool in one launch, stem conv, max pool, conv, block entry (conv1 + downsample in one
 *                launch), average pool + fc
 *   [6] block    BasicBlock 0..15, or -1; [7] conv: 0 conv1 (the block entry too), 1 conv2, 2 the downsample conv, or -1
 *   [8] H, [9] W: the launch's input map; [10] OH, [11] OW: its output map; [12] cin, [13] cout
 *   [14] fmt     bit 0: x is a cell tensor, bit 1: y (both outputs of a block entry), bit 2: the residual; fp32 NCHW otherwise
 *   [15] x, [16] res, [17] y, [18] y2: buffers -- 0..2 the rotating activation regions, 3 the stem region, -1 none (the image, the
 *                feature, no residual); y2: the downsample's output of a block entry.  A segment's tensors start at its first
 *                image's slot of the region's largest map: n0 * 64 * h2 * w2 floats into a rotating region (h2 x w2: the pooled
 *                map), n0 * 64 * h1 * w1 into the stem region (h1 x w1: the stem map).  Workspace, in floats: the stem region,
 *                align64(batch * 64 * h1 * w1), then the three rotating regions of align64(batch * 64 * h2 * w2) each.
 *   [19] scratch_off, [20] scratch_floats: the slice of the stem region lent to the launch as split-reduction scratch, both in
 *                units of 64 floats (0, 0: none -- the region holds the stem map)
 *   [21] status  the launch's status group (adx_resnet_status_name)
 *   [22] nsub, [23] first_split: the forward's sub-batches and the first block that runs per sub-batch (the same in every record) */
#define ADX_RESNET_PLAN_INTS 24
#define ADX_RESNET_PLAN_CAPTURING 1
enum { ADX_RESNET_PLAN_STEM_POOL = 0, ADX_RESNET_PLAN_STEM = 1, ADX_RESNET_PLAN_MAXPOOL = 2, ADX_RESNET_PLAN_CONV = 3,
       ADX_RESNET_PLAN_ENTRY = 4, ADX_RESNET_PLAN_AVGPOOL_FC = 5 };
int adx_resnet_plan_describe(const adx_resnet* r, int32_t batch, int32_t h, int32_t w, int32_t flags, int32_t* n_records, int32_t* ints,
                             int32_t max_records);
/* For tests only, beside adx_resnet_plan_describe (same arguments, same records in the same order; its own record width so that
 * the other's stays what it is): the grid each launch of that plan gets on a device of `cus` compute units.  The pass's persistent
 * 3x3 launches (conv2d_hs3x3q: the 16x16x32 kernel's unit walk) use 8 x ((cus - reserve) / 8) workgroups at most; the reserve is
 * chosen with the sub-batches (ADX_HS_RESERVE_CUS=<n> pins it; so does reserve >= 0 here, -1: the plan's own).  ADX_RESNET_GRID_INTS
 * words per record:
 *   [0] 1: a persistent unit-walk launch, 0: any other (then [1], [2] are 0 and [3] is the grid of a one-tile-per-workgroup 3x3
 *       launch, or 0); [1] units = spatial tiles x cout tiles; [2] workgroups per XCD; [3] grid = 8 x [2]
 *   [4] the plan's reserve, [5] the compute units its launches may use (the same in every record) */
#define ADX_RESNET_GRID_INTS 6
int adx_resnet_plan_grids(const adx_resnet* r, int32_t batch, int32_t h, int32_t w, int32_t flags, int32_t cus, int32_t reserve,
                          int32_t* n_records, int32_t* ints, int32_t max_records);
/* For tests only: the unit walk of a persistent 3x3 launch of `grid` workgroups (a multiple of 8) over `units` = spatial tiles x
 * cout_tiles units, from the range and unit functions the kernel itself uses.  counts[b]: units workgroup b visits (grid words);
 * visits: (spatial tile, cout tile) pairs, workgroup after workgroup in visiting order (2 x units words). */
int adx_conv2d_hs3x3q_walk(int32_t units, int32_t cout_tiles, int32_t grid, int32_t* counts, int32_t* visits);
/* For tests only: the stage walk of the PAIR form of the 4-wave 3x3 stride-1 kernel (16x16x32 MFMAs over two taps x 16 channels) over
 * `nchunks` (even) 16-channel chunks, as events in program order.  Stage -1 is the prologue; a stage ends with a barrier, so what a
 * stage writes to LDS is readable from the next stage on.  ADX_PAIR_EVENT_INTS words per event:
 *   [0] stage  [1] kind  [6] 1: past the end (the last chunk / stage again, into a copy / buffer nobody reads afterwards)
 *   READ     one of the stage's two taps: [2] chunk [3] tap = 3 kh + kw [4] patch copy [5] weight run = 9 chunk + tap; [6] weight buffer
 *   FETCH_P  a patch round requested from memory: [2] chunk [3] round      WRITE_P  ... written to LDS: [2] chunk [3] round [4] copy
 *   FETCH_W  a stage's two weight runs requested: [5] the stage            WRITE_W  ... written to LDS: [4] buffer [5] the stage */
#define ADX_PAIR_EVENT_INTS 7
enum { ADX_PAIR_READ = 0, ADX_PAIR_FETCH_P = 1, ADX_PAIR_WRITE_P = 2, ADX_PAIR_FETCH_W = 3, ADX_PAIR_WRITE_W = 4 };
int adx_conv2d_hs3x3_pair_walk(int32_t nchunks, int32_t* n_events, int32_t* events, int32_t max_events);
int32_t adx_resnet_status_words(const adx_resnet* r);
int adx_resnet_set_status(adx_resnet* r, uint32_t* words /* device, adx_resnet_status_words(r) words, or NULL */);
const char* adx_resnet_status_name(const adx_resnet* r, int32_t group);

/* Op-level 2-D convolution used by the perception executor (one launch): NCHW fp32,
 * y = [relu]( conv(x, w) * scale[c] + shift[c] [+ res] ); scale/shift = eval-mode BatchNorm2d
 * (modeling/resnet.py:87-102).  cout must be a multiple of 64. */
typedef struct adx_conv2d_desc { int32_t cin, cout, k, stride, pad; } adx_conv2d_desc;
size_t adx_conv2d_packed_bytes(const adx_conv2d_desc* d);
int adx_conv2d_pack(const adx_conv2d_desc* d, const float* w /* [cout][cin][k][k] */, float* packed, adx_stream s);
int adx_conv2d_forward(const adx_conv2d_desc* d, const float* x, const float* packed_w, const float* scale,
                       const float* shift, const float* res, float* y, int32_t n, int32_t h, int32_t w,
                       int32_t relu, adx_stream s);
/* The pipelined 3x3 stride-1 kernel can also read and write CELL tensors: per image [C / 8][plane: hi, lo][H][W] cells of
 * 16 bytes = the 8 channels of one pixel split into fp16 halves, x = hi + lo / 2^11 (hi = fp16(x), lo = fp16((x - hi) 2^11)) --
 * the layout its staging writes to LDS, so a consumer copies cells where it would convert fp32 values; same bytes per tensor
 * as fp32 NCHW.  adx_resnet_forward keeps the activations between such launches in this layout (modeling/resnet.py:87-102
 * BasicBlock chain); these two entry points expose the launch for tests and other callers.  fmt: bit 0 = x is a cell tensor,
 * bit 1 = y is (required), bit 2 = res is.  adx_conv2d_cells_supported: 1 when (desc, n, h, w) runs as one such launch. */
int adx_conv2d_cells_supported(const adx_conv2d_desc* d, int32_t n, int32_t h, int32_t w);
/* For tests only (no device needed): what the launch plan of a 3x3 stride-1 conv answers for n x h x w with the operand formats fmt
 * (bits as above; 0: all fp32): out = [family (0 none, 1 conv2d_hs3x3_kernel, 2 the 16x16x32 tile walk), tile mode, parts of a
 * split reduction, 1: the PAIR form, 1: the formats are admitted]. */
int adx_conv2d_hs3x3_plan_query(const adx_conv2d_desc* d, int32_t n, int32_t h, int32_t w, int32_t fmt, int32_t has_res, int32_t* out);
int adx_conv2d_forward_cells(const adx_conv2d_desc* d, const void* x, const float* packed_w, const float* scale,
                             const float* shift, const void* res, void* y, int32_t n, int32_t h, int32_t w, int32_t relu,
                             int32_t fmt, adx_stream s);
/* The entry of a ResNet layer as the inference executor launches it, for tests: conv1 = Conv2d(cin, cout, 3, 2, 1) + BatchNorm
 * (scale1, shift1) + ReLU into y1 and the downsample Conv2d(cin, cout, 1, 2, 0) + BatchNorm (scaled, shiftd) into yd, one launch
 * over x (modeling/resnet.py:87-102, 230-231).  x [n][cin][h][w] and both outputs [n][cout][(h - 1) / 2 + 1][(w - 1) / 2 + 1] are
 * cell tensors (adx_conv2d_forward_cells).  packed_w1: adx_conv2d_pack's image of conv1's weights; packed_wd: adx_conv2d_pack_ds's
 * image of the downsample's [cout][cin][1][1] (cout * cin floats).  Scale / shift pairs may be NULL (identity).  Which kernel runs
 * follows from the shape (cin % 64 == 0 and cout % 128 == 0: the 16x16x32 tile walk over the input's parity planes, else the
 * 32x32x16 kernel); flags bit 0 keeps the launch on the 32x32x16 kernel, as ADX_HS_S2Q=0 does for every launch. */
int adx_conv2d_pack_ds(int32_t cin, int32_t cout, const float* w, float* packed, adx_stream s);
int adx_conv2d_block_s2_cells(int32_t cin, int32_t cout, const void* x, const float* packed_w1, const float* scale1,
                              const float* shift1, void* y1, const float* packed_wd, const float* scaled, const float* shiftd,
                              void* yd, int32_t n, int32_t h, int32_t w, int32_t flags, adx_stream s);
/* The ResNet's stem as the inference executor runs it, for tests: Conv2d(3, 64, 7, 2, 3) + BatchNorm (scale, shift: [64])
 * + ReLU + MaxPool2d(3, 2, 1) in one launch; only the pooled map is written.  x: fp32 NCHW [n][3][h][w], or with x_u8 = 1
 * uint8 camera frames [n][h][w][3] normalised on the fly as (v / 255 - mean) / std (mean, std: three host floats).
 * packed_w: adx_conv2d_pack's image of the stem weights.  y: fp32 [n][64][ph][pw] (ph = (oh - 1) / 2 + 1 of the stem map's
 * oh = (h - 1) / 2 + 1, pw likewise), or with y_cells = 1 the same map as a cell tensor (adx_conv2d_forward_cells).
 * Refused under ADX_CONV_EXACT=1 (it is a split-fp16 kernel). */
int adx_conv2d_stem_pool(const void* x, int32_t x_u8, const float* packed_w, const float* scale, const float* shift,
                         const float* mean, const float* stdv, void* y, int32_t n, int32_t h, int32_t w, int32_t y_cells,
                         adx_stream s);
/* Weight gradient of the same convolution (torch.nn.grad.conv2d_weight; train.py:242 reaches it through
 * loss.backward()): dw [cout][cin][k][k] = sum over batch and pixels of dy (x) x.  dy is [n][cout][oh][ow].
 * scratch: NULL, or >= adx_conv2d_wgrad_scratch_bytes() of device memory in which the range of dy is estimated
 * first -- the 3x3 stride-1 path multiplies on the fp16 matrix cores with hi/lo split operands and rescales dy by an
 * exact power of two; without scratch dy is taken as is (full accuracy only for |dy| >= 6e-5). */
size_t adx_conv2d_wgrad_scratch_bytes(void);
int adx_conv2d_wgrad(const adx_conv2d_desc* d, const float* x, const float* dy, float* dw, int32_t n, int32_t h,
                     int32_t w, void* scratch, adx_stream s);
/* The same with the two uses of the scratch told apart: estimate_range != 0 asks for the range estimate above (scratch
 * required); estimate_range == 0 takes dy as is, and a non-NULL scratch then only carries the per-split copies of the
 * bit-reproducible reduction (ADX_WGRAD_DETERMINISTIC=1; adx_conv2d_wgrad_scratch_bytes() covers both). */
int adx_conv2d_wgrad_ex(const adx_conv2d_desc* d, const float* x, const float* dy, float* dw, int32_t n, int32_t h,
                        int32_t w, void* scratch, int32_t estimate_range, adx_stream s);
/* The same for a 3x3 stride-1 pad-1 convolution with BOTH operands as cell tensors -- how the training executor holds the
 * activations between a BasicBlock's convs and the conv-output gradients (train.py:251, loss.backward()): x_cells
 * [n][cin / 8][hi, lo][h][w] cells, dy_cells likewise over cout, holding dy * dy_scale[0]; dy_scale = two floats {s, 1 / s} on
 * the device, s a power of two.  scratch: NULL, or adx_conv2d_wgrad_scratch_bytes() (ADX_WGRAD_DETERMINISTIC=1). */
int adx_conv2d_wgrad_cells(const adx_conv2d_desc* d, const void* x_cells, const void* dy_cells, const float* dy_scale, float* dw,
                           int32_t n, int32_t h, int32_t w, void* scratch, adx_stream s);

/* Training-mode perception (train.py:242 with model.train()): batch-statistics BatchNorm, running buffers
 * updated in place (momentum 0.1), everything the backward needs kept in the workspace. */
typedef struct adx_resnet_tape adx_resnet_tape;
int adx_resnet_tape_create(adx_resnet_tape** out);
void adx_resnet_tape_destroy(adx_resnet_tape* t);
size_t adx_resnet_train_workspace_bytes(const adx_resnet* r, int32_t batch, int32_t h, int32_t w);
int adx_resnet_forward_train(adx_resnet* r, const float* const* tensors, int32_t n_tensors, void* packed,
                             void* workspace, size_t workspace_bytes, const float* img, int32_t batch, int32_t h,
                             int32_t w, float* feature, adx_resnet_tape* tape, int32_t update_running, adx_stream s);
/* grads: one slot per tensor of adx_resnet_pack's list; conv weight / bn weight / bn bias / fc slots are written,
 * running-statistics slots are ignored (may be NULL). */
int adx_resnet_backward(adx_resnet* r, const float* const* tensors, float* const* grads, int32_t n_tensors,
                        void* workspace, size_t workspace_bytes, adx_resnet_tape* tape, const float* d_feature,
                        adx_stream s);
/* The same with completion events: `events` = adx_resnet_backward_groups(r) hipEvent_t handles (or NULL entries); event g is
 * recorded on `s` behind the last launch that writes a gradient of group g.  Groups in the order the backward produces them:
 * 0 = fc, 1 .. n_blocks = the BasicBlocks from layer4's last to layer1's first, n_blocks + 1 = the stem (conv1 + bn1).
 * adx_resnet_tensor_group(r, i) = the group of tensor slot i (-1: a running statistic).  This is what lets a gradient reduction
 * of the upper layers start while the lower layers are still being differentiated -- what DistributedDataParallel's reducer
 * does per parameter while accelerator.backward(loss) runs (train.py:176-178, 251). */
int32_t adx_resnet_backward_groups(const adx_resnet* r);
int32_t adx_resnet_tensor_group(const adx_resnet* r, int32_t tensor);
int adx_resnet_backward_events(adx_resnet* r, const float* const* tensors, float* const* grads, int32_t n_tensors,
                               void* workspace, size_t workspace_bytes, adx_resnet_tape* tape, const float* d_feature,
                               void* const* events, int32_t n_events, adx_stream s);
/* Fine-tuning: frozen BatchNorm statistics and frozen parameters.
 * adx_resnet_bn_layers(r) = the number of BatchNorm layers (36); adx_resnet_bn_tensor(r, l) = layer l's gamma slot in
 * adx_resnet_pack's list (-1 on a bad index).  Layers are in record order: the stem, then per BasicBlock conv1, [downsample],
 * conv2 (adx_resnet_tape_describe's records).
 * adx_resnet_forward_train_ex: bit l of `frozen_bn` set -> layer l normalises with running_mean / running_var (eps 1e-5) and
 * leaves them untouched (nn.BatchNorm2d in eval mode inside a training forward); the other layers behave as in
 * adx_resnet_forward_train, which is this call with frozen_bn = 0.  A bit >= adx_resnet_bn_layers(r) is refused.
 * adx_resnet_backward_ex: the backward of such a tape, given the same mask (a different one is refused).  A frozen layer
 * backpropagates through its affine map only: dx = gamma rstd_run dy, d gamma = sum dy xhat, d beta = sum dy.  In every
 * adx_resnet_backward* call a NULL conv-weight, gamma, beta or fc slot is a frozen parameter: its gradient is not computed,
 * and nothing below the lowest record that still owns a non-NULL slot runs.  Every group event is still recorded. */
int32_t adx_resnet_bn_layers(const adx_resnet* r);
int32_t adx_resnet_bn_tensor(const adx_resnet* r, int32_t layer);
int adx_resnet_forward_train_ex(adx_resnet* r, const float* const* tensors, int32_t n_tensors, void* packed,
                                void* workspace, size_t workspace_bytes, const float* img, int32_t batch, int32_t h,
                                int32_t w, float* feature, adx_resnet_tape* tape, int32_t update_running, uint64_t frozen_bn,
                                adx_stream s);
int adx_resnet_backward_ex(adx_resnet* r, const float* const* tensors, float* const* grads, int32_t n_tensors,
                           void* workspace, size_t workspace_bytes, adx_resnet_tape* tape, const float* d_feature,
                           uint64_t frozen_bn, void* const* events, int32_t n_events, adx_stream s);
/* For tests only:a read-only description of a tape filled by adx_resnet_forward_train, so that a test can read what the
 * forward kept (and what the backward will condition on) out of the caller's workspace.  Locations are BYTE OFFSETS into
 * `workspace` (the forward's); -1 = none, -2 = outside the forward's part of the workspace (the stem's input: the image).
 * *n_records = the number of conv records (forward launch order: 0 = the stem, then per BasicBlock conv1, [downsample], conv2).
 * index >= 0, record `index`:
 *   ints[12] = {cin, cout, k, stride, pad, H, W, OH, OW, relu, x_cells, out_cells}
 *              relu: 0 none, 1 after the residual add, 2 straight after BatchNorm (the backward re-derives that mask from raw)
 *   offs[7]  = {x, raw, out, identity, mean, rstd, bits}   (bits: byte [n][c / 8][pixel], bit c % 8, of the output's mask)
 * index == -1, the tape:
 *   ints[12] = {n_records, batch, h, w, ph, pw, poh, pow, fh, fw, 0, 0}   (stem map, pooled map, final map sizes)
 *   offs[7]  = {pool_code, pool_out, final_map, -1, -1, -1, -1}           (pool_code: first-maximum tap ty * 3 + tx per window)
 * Refuses (ADX_ERR_*) a null tape / workspace / output, a tape with no forward and an index out of range. */
int adx_resnet_tape_describe(const adx_resnet_tape* tape, const void* workspace, int32_t index, int32_t* n_records,
                             int32_t* ints, int64_t* offs);

/* ------------------------------------------------------------------------------------
 * Classifier guidance: TrajPredict state head (modeling/helpers.py:22-59; hidden 64, 4 heads,
 * ff 256, 2 layers, eval mode) forward, input gradient, and the fused guidance update.
 * -----------------------------------------------------------------------------------*/
typedef struct adx_trajpred adx_trajpred;
int adx_trajpred_create(int32_t out_dim, adx_trajpred** out);
void adx_trajpred_destroy(adx_trajpred* t);
int adx_trajpred_num_params(const adx_trajpred* t);       /* state_pred.* named_parameters() count (30) */
size_t adx_trajpred_packed_bytes(const adx_trajpred* t);
/* Sequence lengths: T = horizon - 1 from 1 to 63 (modeling/temporal.py:119 builds the head for any horizon).  T <= 31 keeps
 * every activation of a sample in LDS; T = 32..63 runs a 64-row instantiation that keeps three large tiles per sample in
 * a scratch the caller lends (no initialisation; alive and unshared while launches that use it are in flight).
 * adx_trajpred_scratch_bytes is 0 for T <= 31; the calls below fail with ADX_ERR_STATE when the lent scratch is too small. */
size_t adx_trajpred_scratch_bytes(const adx_trajpred* t, int32_t batch, int32_t T);
int adx_trajpred_set_scratch(adx_trajpred* t, void* scratch, size_t bytes);
int adx_trajpred_pack(adx_trajpred* t, const float* const* params, int32_t n, const float* freqs, void* packed,
                      adx_stream s);
/* out[B][T][out_dim] = state_pred(action[B][T][3] (strides act_sb, act_st), time_embed[B][64]) */
int adx_trajpred_forward(adx_trajpred* t, const void* packed, const float* action, int64_t act_sb, int64_t act_st,
                         const float* time_embed, float* out, int32_t batch, int32_t T, adx_stream s);
/* grad_action[B][T][3] = (d out / d action)^T grad_out[B][T][out_dim]; what torch.autograd.grad returns for
 * `action` in control/guidance.py:47-50 through the state path */
int adx_trajpred_backward(adx_trajpred* t, const void* packed, const float* action, int64_t act_sb, int64_t act_st,
                          const float* time_embed, const float* grad_out, float* grad_action, int32_t batch,
                          int32_t T, adx_stream s);
/* Training (train.py:242-251 with CLASSIFIER_GUIDANCE): parameter gradients of the state head.  grad_image has
 * the layout of the packed buffer (adx_trajpred_packed_bytes); parameter i lives at float offset
 * offsets[i] (adx_trajpred_param_offsets, adx_trajpred_pack order) in its PyTorch layout. */
int adx_trajpred_backward_params(adx_trajpred* t, const void* packed, const float* action, int64_t act_sb,
                                 int64_t act_st, const float* time_embed, const float* grad_out, float* grad_action,
                                 void* grad_image, float* d_time_embed, int32_t batch, int32_t T, float dropout_p,
                                 uint64_t seed, adx_stream s);
/* Train-mode forward of the state head: nn.TransformerEncoderLayer's dropout (modeling/helpers.py:35-41 leaves it at
 * torch's default 0.1: attention probabilities, both residual branches, the feed-forward activation) with masks that are
 * a pure function of (seed, sample, site, element) -- adx_trajpred_backward_params regenerates them from the same
 * (dropout_p, seed).  dropout_p = 0 is the deterministic path the golden fixtures use. */
int adx_trajpred_forward_train(adx_trajpred* t, const void* packed, const float* action, int64_t act_sb, int64_t act_st,
                               const float* time_embed, float* out, int32_t batch, int32_t T, float dropout_p,
                               uint64_t seed, adx_stream s);
int adx_trajpred_param_offsets(const adx_trajpred* t, int64_t* offsets, int32_t n);
/* One launch for interact.py:153-160 + GuidanceLoss.forward with STEP = 1 (control/guidance.py:35-59) +
 * TargetGuidance (control/guidance_loss.py:10-22), per sample:
 * x = cat([0; state_pred(action[:-1])], action); pick h*; x -= scaled gradient; clip(-1, 1). */
int adx_guided_output(adx_trajpred* t, const void* packed, const float* action /* [B][T+1][3] */,
                      const float* time_embed, const float* target /* [B][2] */, float model_std, float scale,
                      float* x_guided /* [B][T+1][out_dim+3] */, float* loss /* [B] or NULL */, int32_t batch,
                      int32_t T, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Optimizer step of train.py:252-261 in one launch: grad nan_to_num, AdamW, EMA shadow update.
 * table = device array of {float* p; const float* g; float* m; float* v; float* ema; int64_t n} per tensor;
 * block_tensor / block_chunk map each workgroup to (tensor, chunk of adx_optim_chunk() elements).
 * -----------------------------------------------------------------------------------*/
int adx_optim_chunk(void);
int adx_adamw_ema_step(const void* table, const int32_t* block_tensor, const int32_t* block_chunk, int32_t n_blocks,
                       float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                       float ema_decay, int32_t use_ema, int32_t sanitize, adx_stream s);
/* the same with every gradient multiplied by grad_scale as it is read (data-parallel training: 1 / world_size when the
 * all-reduce left the SUM over the ranks in .grad; the reference's DDP divides inside its own reduction, train.py:176-178) */
int adx_adamw_ema_step_scaled(const void* table, const int32_t* block_tensor, const int32_t* block_chunk, int32_t n_blocks,
                       float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                       float ema_decay, int32_t use_ema, int32_t sanitize, float grad_scale, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Scheduler step math.  The integer schedule and the fp32 scalar coefficients are computed
 * by the host (the scheduler/ modules keep them as 0-dim CPU tensors) and passed by value.
 * -----------------------------------------------------------------------------------*/
#define ADX_PRED_EPSILON 0
#define ADX_PRED_SAMPLE 1
#define ADX_PRED_V 2

typedef struct adx_step_coef {
  int32_t prediction_type;     /* ADX_PRED_* */
  int32_t clip;                /* 1: clamp x0 to [-clip_range, clip_range]; `thresholding=True` with the
                                  diffusers default sample_max_value=1 is exactly clamp(-1, 1) */
  float clip_range;
  float sqrt_alpha_t, sqrt_beta_t;   /* abar_t ** 0.5, (1 - abar_t) ** 0.5 */
  float c_x0;                  /* DDIM: abar_prev ** 0.5;  DDPM: pred_original_sample_coeff */
  float c_dir;                 /* DDIM: (1 - abar_prev - std^2) ** 0.5 */
  float c_x;                   /* DDPM: current_sample_coeff */
  float c_noise;               /* DDIM: std_dev_t = eta * var ** 0.5;  DDPM: var ** 0.5 */
  int32_t add_noise;           /* DDIM: eta > 0;  DDPM: t > 0 */
  int32_t use_clipped_model_output;
  /* inpainting schedulers only */
  int32_t inpaint;             /* 1: Inpainting*Scheduler arithmetic */
  float c_const;               /* inpainting DDIM quirk: the SCALAR variance is added to every element */
  float c_known, c_known_noise;/* RePaint: known = c_known * target + (known_noise ? c_known_noise * z : 0) */
  int32_t known_noise;         /* t > 0 */
  /* classifier-free guidance combine fused in front of the step (interact.py:142-144):
   * model_output = uncond + free_scale * (cond - uncond); rows [0,B) cond, [B,2B) uncond */
  int32_t cfg_combine; float free_scale;
  int32_t zero_first;          /* 1: prev[:, 0, :3] = 0 after the step (interact.py:164, train.py:88) */
} adx_step_coef;

/* S1/S3: GuidanceDDIMScheduler.step / InpaintingDDIMScheduler.step
 *        scheduler/guidance_ddim_scheduler.py:60-173, inpainting_ddim_scheduler.py:10-153
 * Refused, as by every step export below: batch * horizon * dim above 0x3fffffff, more elements than the kernel's 32-bit
 * index holds. */
int adx_ddim_step(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                  const float* target, const float* mask, float* prev, float* x0,
                  int32_t batch, int32_t horizon, int32_t dim, adx_stream s);
/* S2/S4: GuidanceDDPMScheduler.step / InpaintingDDPMScheduler.step / stock DDPMScheduler.step
 *        scheduler/guidance_ddpm_scheduler.py:59-178, inpainting_ddpm_scheduler.py:10-146, train.py:87 */
int adx_ddpm_step(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                  const float* target, const float* mask, float* prev, float* x0,
                  int32_t batch, int32_t horizon, int32_t dim, adx_stream s);
/* DPM-Solver++ multistep step, orders 1 and 2 (midpoint).  No reference counterpart: the reference names a "dpm" scheduler
 * (interact.py:92-93) but never constructs one; the arithmetic is diffusers 0.28.0 DPMSolverMultistepScheduler with
 * algorithm_type = "dpmsolver++", restated on the host in scheduler/dpm.py.  With sigma_i the schedule's noise level at
 * step i (sigma = 0 after the last step), alpha = 1 / sqrt(sigma^2 + 1), sigma_t = sigma * alpha, lambda = log(alpha) -
 * log(sigma_t) and h = lambda_{i+1} - lambda_i, the host passes fp32 scalars by value; the kernel rounds every product on its
 * own, left to right:
 *   m     = cfg_combine ? uncond + free_scale * (cond - uncond) : model_output      (rows [0,B) cond, [B,2B) uncond)
 *   x0    = epsilon: (x - sigma_s * m) / alpha_s;  sample: m;  v_prediction: alpha_s * x - sigma_s * m;  then the clamp
 *   prev  = r * x - k * x0                                                           first order (== a DDIM step)
 *   prev  = (r * x - k * x0) - half_k * (inv_r0 * (x0 - prev_x0))                    second_order, prev_x0 given
 * The last step of a schedule has sigma_{i+1} = 0: h = inf, r = 0, k = -1, i.e. prev = x0. */
typedef struct adx_dpm_coef {
  int32_t prediction_type;     /* ADX_PRED_* */
  int32_t clip;                /* 1: clamp x0 to [-clip_range, clip_range] (`thresholding=True`, sample_max_value = 1) */
  float clip_range;
  float alpha_s, sigma_s;      /* alpha and sigma * alpha at the CURRENT step i */
  float r;                     /* sigma_t(i+1) / sigma_t(i) */
  float k;                     /* alpha(i+1) * (exp(-h) - 1) */
  int32_t second_order;        /* 1: add the multistep term; needs prev_x0 */
  float inv_r0;                /* 1 / r0, r0 = (lambda_i - lambda_{i-1}) / h */
  float half_k;                /* 0.5 * k */
  int32_t cfg_combine; float free_scale;   /* as in adx_step_coef */
  int32_t zero_first;          /* 1: prev[:, 0, :3] = 0 on prev_sample only; x0 is written as computed */
} adx_dpm_coef;

/* model_output: [batch][horizon][dim], or [2 * batch] rows when c->cfg_combine.  prev_x0: the x0 the previous step wrote, or
 * NULL (then the step is first order; NULL with c->second_order set is refused).  prev_sample and x0 are both always
 * written and may not alias an input: x0 is the next step's prev_x0. */
int adx_dpm_step(const adx_dpm_coef* c, const float* model_output, const float* sample, const float* prev_x0,
                 float* prev_sample, float* x0, int32_t batch, int32_t horizon, int32_t dim, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Noise stream v1: standard normals as a pure function of (seed, tick, slot, element).  No reference counterpart (the
 * reference draws torch.randn per step); the values differ from torch's for the same seed.  Fixtures and users depend on
 * this definition -- a change is a new stream version, never an edit.
 *
 *   words    Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85),
 *            key = (seed low 32, seed high 32), counter = (e >> 2, slot, tick low 32, tick high 32) -> w0..w3
 *   e        the element's flat index in the LOGICAL tensor [rows][H][D]: e = ((row_offset + b) * H + h) * D + d; never a
 *            thread or tile index, so the values do not move with the launch shape or with how rows are sharded.
 *            e >> 2 must fit 32 bits: e < 2^34, refused otherwise.
 *   slot     the integer timestep t the scheduler step is taken at; ADX_NOISE_INIT_SLOT for the initial trajectory
 *   normals  u_i = ((w_i >> 8) + 0.5) * 2^-24 in (0, 1);  r = sqrt(-2 ln u0), z0 = r cos(2 pi u1), z1 = r sin(2 pi u1);
 *            z2, z3 the same from (u2, u3).  Element e takes z[e & 3] (adx_noise_words: w[e & 3]).  Accurate fp32 maths.
 *   state    four 32-bit words {seed_lo, seed_hi, tick_lo, tick_hi} in DEVICE memory.  Every kernel reads them through the
 *            pointer when it runs, so a captured graph draws under the values current at each replay.
 * -----------------------------------------------------------------------------------*/
#define ADX_NOISE_INIT_SLOT (-1)   /* slot 0xFFFFFFFF */
#define ADX_NOISE_STATE_WORDS 4

/* out[i] = the stream's normal / raw word of logical element first_elem + i, i in [0, n), under the state's current seed and
 * tick; first_elem and n need not be multiples of 4.  Exactly what a *_step_rng kernel draws at those elements. */
int adx_noise_normal(const uint32_t* state, int32_t slot, int64_t first_elem, float* out, int64_t n, adx_stream s);
int adx_noise_words(const uint32_t* state, int32_t slot, int64_t first_elem, uint32_t* out, int64_t n, adx_stream s);
/* tick += 1 (64-bit) by a one-thread kernel on the stream: capturable, ordered with the draws around it */
int adx_noise_advance(uint32_t* state, adx_stream s);
/* adx_ddim_step / adx_ddpm_step with the noise tensor replaced by the stream: element (b, h, d) of the launch draws logical
 * element ((row_offset + b) * H + h) * D + d of `slot`, inside the step kernel, only where the step uses noise.  Refused: what
 * adx_ddim_step refuses (the 32-bit element count included), a NULL noise_state, rows that leave the stream's 2^34 elements. */
int adx_ddim_step_rng(const adx_step_coef* c, const float* model_output, const float* sample, const uint32_t* noise_state,
                      int32_t slot, int64_t row_offset, const float* target, const float* mask, float* prev, float* x0,
                      int32_t batch, int32_t horizon, int32_t dim, adx_stream s);
int adx_ddpm_step_rng(const adx_step_coef* c, const float* model_output, const float* sample, const uint32_t* noise_state,
                      int32_t slot, int64_t row_offset, const float* target, const float* mask, float* prev, float* x0,
                      int32_t batch, int32_t horizon, int32_t dim, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Selection cost v1: best-of-K sampling.  K candidate trajectories per scene are scored and the best one is copied out, in
 * one launch with no host decision (a node of a captured graph).  No reference counterpart: train.evaluate draws many
 * trajectories for one image only to paint them (train.py:62-90).  Callers and fixtures depend on this definition -- a
 * change is a new cost version, never an edit.
 *
 *   layout   trajs [candidates * scenes][H][D], CANDIDATE-MAJOR: candidate k of scene s is row k * scenes + s -- the row
 *            order of a sampling loop whose image batch is `scenes` (adx_embed_forward: row r reads feature r % feat_rows).
 *   points   p_h = (x, y) = the first min(D, 2) columns of waypoint h, h = 0..H-1; a missing y column (D = 1) counts as 0.
 *            Units are the model's own: the clamped trajectory BEFORE any xy scaling, the units of `target`.
 *   goal     min over h of |p_h - g_s|^2, g_s = target[s].  0 when target is NULL; w_goal is then ignored.
 *   smooth   mean over h = 1..H-2 of |p_{h+1} - 2 p_h + p_{h-1}|^2; 0 when H < 3.
 *   consensus  mean over h of |p_h - m_h|^2, m_h = the mean of p_h over the scene's K candidates.
 *   cost     w_goal * goal + w_smooth * smooth + w_consensus * consensus, in this order.  A term whose weight is exactly 0
 *            is not evaluated: it contributes 0 whatever its value would be (a NaN candidate then cannot reach the others'
 *            costs through the mean path of a consensus term nobody asked for).  A NaN waypoint makes every term it enters NaN.
 *   index    index[s] = the smallest k with the smallest cost.  A non-finite cost (NaN, +-inf) loses to every finite one;
 *            if no cost of the scene is finite, index[s] = 0.
 *   best     best[s] = row index[s] * scenes + s of trajs, all H * D values, copied bit for bit.
 *   arithmetic  fp32, every product and sum rounded on its own, fixed reduction trees, no atomics: the same input gives the
 *            same bits on every launch.  cost is defined up to fp32 rounding of the sums above (tests/select_ref.py restates
 *            it in fp64 and derives the bound), index and best exactly wherever the two smallest costs differ by more than that.
 *
 * Limits: 1 <= candidates <= 64, 1 <= horizon <= 64 (the longest the UNet takes), 1 <= dim <= 16, 1 <= scenes <= 65535.
 * ADX_ERR_INVALID before any GPU work for a value out of range, a NULL pointer other than target, or an output that
 * overlaps trajs or another output.
 * -----------------------------------------------------------------------------------*/
typedef struct adx_select_cfg {
  int32_t scenes, candidates, horizon, dim;
  float w_goal, w_smooth, w_consensus;
} adx_select_cfg;
/* trajs [candidates*scenes][H][D], row = k*scenes + s; target [scenes][2] or NULL; cost [scenes][candidates];
 * index [scenes] (int32); best [scenes][H][D].  No output may alias trajs. */
int adx_traj_select(const adx_select_cfg* c, const float* trajs, const float* target, float* cost, int32_t* index,
                    float* best, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Warm start v1: a sampling tick's initial trajectory from the previous tick's result (receding-horizon warm starting).
 * One launch, one thread per output element, no host decision; the stream's state is read through the pointer, so the call
 * can be a node of a captured graph.  No reference counterpart: the reference's agents start every tick from noise
 * (e2e_driving/diffusion_agent.py:94,181).  Callers and fixtures depend on this definition -- a change is a new version,
 * never an edit.
 *
 *   prev     [prev_rows][H][D]: the last tick's result in the model's own units -- the clamped trajectory BEFORE xy scaling,
 *            the units of selection cost v1.  Columns: 0, 1 = x, y; 2 = yaw relative to the first waypoint; 3.. = speed, controls.
 *   rows     a multiple of prev_rows; output row r reads prev[r % prev_rows] (candidate-major: every candidate of a scene
 *            starts from that scene's last winner).
 *   shift    0 <= shift <= H - 1: the waypoints passed since the last tick.
 *   motion   [prev_rows][3] = (tx, ty, phi), the caller's odometry in model units and radians, or NULL.
 *   arithmetic  fp32, no contraction, every product and sum rounded on its own, in this order:
 *     advance  j = h + shift.  j <= H-1: u[h][d] = prev[j][d].  Otherwise d < 2: u[h][d] = prev[H-1][d] +
 *              (float)(j - (H-1)) * (prev[H-1][d] - prev[H-2][d]);  d >= 2: u[h][d] = prev[H-1][d] (the tail is held).
 *     re-base  with o = prev[shift].  motion NULL: w = u[h][d] - o[d] for d < min(D, 3); columns d >= 3 are u unchanged (no
 *              rotation is evaluated, nothing is multiplied by 1).  With motion: qx = u[h][0] - tx, qy = u[h][1] - ty (a
 *              missing y column counts as 0), c = cosf(phi), s = sinf(phi), x' = c * qx + s * qy, y' = -(s * qx) + c * qy;
 *              column 2 is still u - o[2].
 *     clamp    to [-1, 1]; NaN propagates.
 *     noise    v = sqrt_ab * w + sqrt_1mab * z, z = the stream's normal at slot ADX_NOISE_INIT_SLOT and logical element
 *              ((row_offset + r) * H + h) * D + d (a warm tick makes no cold initial draw: the slot is free in that tick).
 *     zero_first != 0: v = 0 where h == 0 && d < 3.
 *   sqrt_ab, sqrt_1mab: sqrt(abar_tau), sqrt(1 - abar_tau) of the level tau the schedule's suffix starts at, by value.
 *
 * ADX_ERR_INVALID before any GPU work: H outside 2..64, D outside 1..16, shift outside 0..H-1, rows not a positive multiple of
 * prev_rows, rows that leave the stream's 2^34 elements, more elements than the kernel's 32-bit index holds, a NULL pointer
 * other than motion, an output that overlaps prev.
 * -----------------------------------------------------------------------------------*/
int adx_warm_init(const float* prev, int32_t prev_rows, const float* motion, float* out, int32_t rows, int32_t horizon,
                  int32_t dim, int32_t shift, float sqrt_ab, float sqrt_1mab, const uint32_t* noise_state, int64_t row_offset,
                  int32_t zero_first, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Pinned waypoints v1: waypoints the caller has already decided, held through a sampling tick while the sampler plans the rest
 * around them (a commit horizon, a stop point, a fixed hand-over).  The reference's loops pin one cell group this way -- after
 * every step they overwrite [:, 0, :3] with its clean value (interact.py:164, train.py:88; Diffuser's apply_conditioning) --
 * and its Inpainting*Scheduler classes hold the RePaint blend, which no caller constructs; this is the first made general, with
 * the second as a mode of the same arithmetic.  A compile-time variant of the step kernels, no host decision: a node of a
 * captured graph.  Callers and fixtures depend on this definition -- a change is a new version, never an edit.
 *
 *   known    [known_rows][H][D] in the model's own units: the units of `target` and of the clamped result BEFORE xy scaling.
 *   mask     [known_rows][H][D], float: 1 = pinned, 0 = free, values between blend linearly; values outside [0, 1] are the
 *            caller's business.
 *   rows     row r of a launch of `batch` rows reads known row r % known_rows (candidate-major, as the conditioning table reads
 *            features: every candidate of a scene carries that scene's pins); batch % known_rows == 0.
 *   per step on the finished prev_sample -- after the sampler's update and after the step's own noise term where it has one,
 *            before zero_first, which keeps the last word on waypoint 0:
 *              kp   = c_known * known + (known_noise ? c_known_noise * z : 0)
 *              prev = mask * kp + (1 - mask) * prev              u = mask * kp;  v = (1 - mask) * prev;  prev = u + v
 *            fp32, no contraction, every product and sum rounded on its own, as written.
 *   z        the step's noise at that element, the very value the step's own noise term uses; no second draw is made.  Tensor
 *            path: element e of the noise tensor.  Stream path: the stream's normal at slot = the step's integer timestep and
 *            logical element e = ((row_offset + b) * H + h) * D + d (adx_pin_apply: slot ADX_NOISE_INIT_SLOT).
 *   x0       pred_original_sample is written as computed and is never pinned: it is the DPM solver's history.
 *   modes    host scalars only; the kernel knows none.
 *     clean    c_known = 1, known_noise = 0: the reference loop's idiom.  Needs no noise; the step stays deterministic.
 *     repaint  (c_known, c_known_noise, known_noise) = the level the step lands on.  DDIM / DDPM: sqrt(abar_prev),
 *              sqrt(1 - abar_prev), t > 0 (the c_known, c_known_noise, known_noise of adx_step_coef, which the pinned step
 *              does not read).  DPM: alpha and sigma * alpha of sigma_{i+1}, known_noise = (i < n - 1).
 *   consequences  with finite operands mask == 1 gives prev == kp and mask == 0 leaves prev as it was, bit for bit (up to the
 *            sign of a zero: x + 0 is +0 for x = -0).  The last step of every schedule lands on the clean level in both modes
 *            (abar_prev = 1 with set_alpha_to_one, sigma = 0), so after the loop's clamp(-1, 1) a pinned cell equals `known`
 *            exactly when |known| <= 1 and the cell is not one zero_first writes.
 *
 * ADX_ERR_INVALID before any GPU work: NULL known or mask, known_rows < 1 or not dividing batch, both a noise tensor and a noise
 * state, known_noise set with neither, c->inpaint together with a pin, an output that overlaps known or mask, more elements than
 * the kernel's 32-bit index holds, rows that leave the stream's 2^34 elements, and whatever the unpinned step refuses.
 * -----------------------------------------------------------------------------------*/
typedef struct adx_pin {
  const float* known;          /* [known_rows][H][D] */
  const float* mask;           /* [known_rows][H][D] */
  int32_t known_rows;
  float c_known, c_known_noise;
  int32_t known_noise;
} adx_pin;
/* adx_ddim_step(_rng) / adx_ddpm_step(_rng) with the blend above.  `noise`: the step's noise tensor or NULL; `noise_state`: the
 * stream's state or NULL (then slot and row_offset are not read); at most one of the two.  A NULL pin is exactly the unpinned
 * export of the noise source given (target = mask = NULL). */
int adx_ddim_step_pin(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                      const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, float* prev, float* x0,
                      int32_t batch, int32_t horizon, int32_t dim, adx_stream s);
int adx_ddpm_step_pin(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                      const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, float* prev, float* x0,
                      int32_t batch, int32_t horizon, int32_t dim, adx_stream s);
/* adx_dpm_step with the blend: the one DPM path that can draw (known_noise), from the stream only.  A NULL pin is adx_dpm_step. */
int adx_dpm_step_pin(const adx_dpm_coef* c, const float* model_output, const float* sample, const float* prev_x0,
                     const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, float* prev_sample,
                     float* x0, int32_t batch, int32_t horizon, int32_t dim, adx_stream s);
/* The blend alone, in place on x [batch][H][D]; z, if pin->known_noise, from the stream at ADX_NOISE_INIT_SLOT. */
int adx_pin_apply(float* x, const adx_pin* pin, const uint32_t* noise_state, int64_t row_offset, int32_t batch, int32_t horizon,
                  int32_t dim, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Cost guidance v1: where NOT to go.  Analytic cost guidance on the predicted clean trajectory (Diffuser-style test-time
 * steering): every sampler step moves the xy of its pred_original_sample down the gradient of a cost of moving discs and
 * half-planes, inside the step kernel, and derives the rest of the step from the moved x0 -- how the reference's classifier
 * guidance acts for its own PRED_TYPE = "sample".  The reference names the idea (GUIDANCE.LOSS_LIST, one entry, under
 * CLASSIFIER_GUIDANCE only); as a caller-facing object it has no counterpart.  A compile-time variant of the step kernels, no
 * host decision: a node of a captured graph.  Callers and fixtures depend on this definition -- a change is a new version,
 * never an edit.
 *
 * Everything is in the model's own units (the units of `target` and of the clamped result BEFORE xy scaling) and in this tick's
 * ego frame.
 *
 *   discs    [scene_rows][M][5] = (cx, cy, vx, vy, r), 0 <= M <= 32.  At waypoint h the centre is (cx + h * vx, cy + h * vy), h
 *            converted to float.  A slot is empty unless r > 0 (a NaN or negative radius is an empty slot).
 *   planes   [scene_rows][P][3] = (nx, ny, b), 0 <= P <= 8: the half-plane nx * x + ny * y <= b.  The normal is not normalised by
 *            the kernel; an all-zero normal contributes a zero gradient by itself.
 *   rows     row r of a launch of `batch` rows reads scene r % scene_rows (candidate-major, as the pin and the conditioning
 *            table); batch % scene_rows == 0.
 *   cost     of one waypoint p = (x, y) at index h: fp32, no contraction, every operation rounded on its own, in this order,
 *            from J = gx = gy = 0, discs in index order and then planes in index order:
 *              disc:   ox = cx + h * vx;  oy = cy + h * vy;  dx = x - ox;  dy = y - oy;  d2 = dx * dx + dy * dy
 *                      inv = 1 / (r * r);  phi = 1 - d2 * inv;  active iff phi > 0
 *                      J = J + (phi * phi) / 2;  k = (2 * phi) * inv;  gx = gx - k * dx;  gy = gy - k * dy
 *              plane:  psi = (nx * x + ny * y) - b;  active iff psi > 0
 *                      J = J + (psi * psi) / 2;  gx = gx + psi * nx;  gy = gy + psi * ny
 *            No square root and no singular point: on a disc's centre the term is active with a zero gradient.  Every comparison
 *            with a NaN is false, so that term is inactive.
 *   per step inside the step kernel, for columns d < 2 only (columns d >= 2 take the unguided path untouched).  From p = the
 *            step's pred_original_sample of the waypoint's two xy elements, after the step's own clip; then for it = 0..iters-1,
 *            1 <= iters <= 8:
 *              g  = the gradient above at p
 *              sh = clamp(lambda * g, -cap, +cap)      componentwise; clamp(v, lo, hi) = v < lo ? lo : (v > hi ? hi : v)
 *              p  = p - sh
 *              if c->clip: p = clamp(p, -clip_range, +clip_range)
 *            cap may be +inf.  The cost couples nothing across waypoints, so the iterations are local to a thread; the x thread
 *            and the y thread of a waypoint repeat the same sequence (each recomputes its partner's x0) and agree.
 *   moved    an element moves iff its own component of sh compared unequal to 0 in some iteration (a NaN does).  A moved
 *            element uses its component of the final p as its x0 everywhere after this point:
 *              DDIM   c_x0 * x0 + c_dir * eps, eps re-derived as (x - sqrt_alpha_t * x0) / sqrt_beta_t: exactly the
 *                     use_clipped_model_output arithmetic;
 *              DDPM   c_x0 * x0 + c_x * x;
 *              DPM    the first- and second-order terms;
 *            and its x0 output is the guided value: the 2M solver's history.  An element that did not move runs the unguided
 *            step, bit for bit (its x0 is the value before the iterations, whatever the sign of a zero became in them).
 *   order    classifier-free combine (when fused; the partner element's model output is combined the same way), x0, clip, guide,
 *            sampler update, noise, pin blend, zero_first.  Waypoint 0 is guided like any other; zero_first keeps the last word
 *            on prev.
 *   lambda   a host scalar by value; the kernel knows no schedule.  `constant`: lambda = fp32(scale).  `variance`: lambda =
 *            fp32(scale) * (sb * sb) in fp32, sb = sqrt_beta_t for DDIM / DDPM and sigma_s for DPM: guidance fades as the sample
 *            gets clean (Diffuser's Sigma-scaling).
 *
 * ADX_ERR_INVALID before any GPU work, each with its own text: dim < 2; M or P out of range; a NULL array with a nonzero count;
 * scene_rows < 1 or not dividing batch; iters out of range; cap negative or NaN; lambda NaN; c->inpaint together with a guide;
 * an output overlapping discs or planes; and whatever the unguided (pinned) step refuses.
 * -----------------------------------------------------------------------------------*/
#define ADX_GUIDE_MAX_DISCS 32
#define ADX_GUIDE_MAX_PLANES 8
#define ADX_GUIDE_MAX_ITERS 8
typedef struct adx_guide {
  const float* discs;          /* [scene_rows][n_discs][5], or NULL with n_discs == 0 */
  const float* planes;         /* [scene_rows][n_planes][3], or NULL with n_planes == 0 */
  int32_t scene_rows, n_discs, n_planes;
  int32_t iters;
  float lambda, cap;
} adx_guide;
/* adx_ddim_step_pin / adx_ddpm_step_pin / adx_dpm_step_pin with the guidance above; pin and guide may each be NULL.  A NULL guide
 * is exactly the _pin export. */
int adx_ddim_step_guide(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                        const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                        float* prev, float* x0, int32_t batch, int32_t horizon, int32_t dim, adx_stream s);
int adx_ddpm_step_guide(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                        const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                        float* prev, float* x0, int32_t batch, int32_t horizon, int32_t dim, adx_stream s);
int adx_dpm_step_guide(const adx_dpm_coef* c, const float* model_output, const float* sample, const float* prev_x0,
                       const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                       float* prev_sample, float* x0, int32_t batch, int32_t horizon, int32_t dim, adx_stream s);
/* What a plan still violates: cost[r] = the cost above summed over row r's waypoints, active[r] = the number of active
 * (waypoint, constraint) pairs, of traj [rows][H][D] (2 <= D, H <= 64; row r reads scene r % scene_rows).  iters, lambda and cap
 * are not read.  Per waypoint J is accumulated as written above; the H values are then summed by a fixed xor butterfly over a
 * 64-lane wave (offsets 32, 16, .. 1; lanes h >= H hold 0): the same input gives the same bits, and cost is defined up to fp32
 * rounding of that sum (tests/guide_ref.py restates it in fp64 and derives the bound).  Refused: a NULL pointer, H outside 1..64,
 * D < 2, the guide's own shape refusals above, an output overlapping traj, discs, planes or the other output. */
int adx_guide_cost(const float* traj, const adx_guide* guide, float* cost, int32_t* active, int32_t rows, int32_t horizon,
                   int32_t dim, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Selection cost v2: best-of-K selection that sees the guide.  Selection cost v1 with one more term -- what a candidate still
 * violates of the scene's discs and planes -- and a hard rule: a candidate that violates nothing beats every candidate that
 * violates something.  One launch, the launch that already holds every candidate's xy on chip, no host decision (a node of a
 * captured graph).  Selection cost v1, adx_traj_select and adx_select_cfg stay as they are; this stands beside them.  Callers and
 * fixtures depend on this definition -- a change is a new version, never an edit.
 *
 * From selection cost v1, word for word: the layout (candidate-major rows), the points and units, the goal, smooth and consensus
 * terms and their arithmetic, "a weight of exactly 0 is not evaluated", the copy of `best` bit for bit, the limits on candidates,
 * horizon and scenes, and the arithmetic (fp32, every operation rounded on its own, fixed trees, no atomics: the same input gives
 * the same bits on every launch).
 *
 *   violation  violation[s][k] = the cost J of cost guidance v1 of candidate k's waypoints under scene s's discs and planes: per
 *              waypoint exactly as that contract writes it, with h = the waypoint index; the H values summed by the fixed xor
 *              butterfly of adx_guide_cost (lane = waypoint, lanes h >= H hold 0).  So violation[s][k] is bit for bit
 *              adx_guide_cost's cost[k * scenes + s] on the same trajs and guide.
 *   active     active[s][k] (int32) = adx_guide_cost's active[k * scenes + s], exactly.  Always written, whatever the weights.
 *   cost       ((w_goal * goal + w_smooth * smooth) + w_consensus * consensus) + w_guide * violation: v1's sum in v1's order, the
 *              new term last.  w_guide == 0: the term is not evaluated.
 *   free       free[s][k] = active[s][k] == 0 AND every x and y of the candidate is finite.  (A NaN waypoint compares false
 *              against every constraint and would otherwise count as "violates nothing": a plan with a NaN in it never wins on
 *              safety grounds.)
 *   index      hard == 0: v1's rule on cost.  hard != 0: if at least one candidate of the scene is free and has a finite cost,
 *              v1's rule over those candidates alone; otherwise v1's rule over all candidates.  v1's rule: the smallest k among
 *              the smallest finite costs; no finite cost -> 0.
 *   blocked    blocked[s] (int32) = 1 if the chosen candidate is not free, else 0.  Written in both modes.
 *   guide      not NULL.  n_discs == n_planes == 0 is legal: everything is then free unless non-finite.  scene_rows equals
 *              `scenes`, or is 1 for a guide without discs and planes.  iters, lambda and cap are not read.
 *
 * ADX_ERR_INVALID before any GPU work, each with its own text: v1's refusals; dim < 2; a NULL guide, active or blocked; the
 * guide's own shape refusals (the check of adx_guide_cost); scene_rows that is neither of the two above; an output overlapping
 * trajs, discs, planes or another output.
 * -----------------------------------------------------------------------------------*/
typedef struct adx_select_guide_cfg {
  int32_t scenes, candidates, horizon, dim;
  float w_goal, w_smooth, w_consensus, w_guide;
  int32_t hard;
} adx_select_guide_cfg;
/* trajs, target, cost, index, best as adx_traj_select; active [scenes][candidates] and blocked [scenes] (int32). */
int adx_traj_select_guide(const adx_select_guide_cfg* c, const float* trajs, const float* target, const adx_guide* guide,
                          float* cost, int32_t* active, int32_t* index, int32_t* blocked, float* best, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Cost guidance v2: cost guidance v1 plus a FIELD term -- a cost raster a perception stack produces (drivable area, kerbs,
 * parked-car blobs), read bilinearly at every waypoint.  v1 stays as it is: adx_guide, the _guide exports and their bits; v2
 * stands beside it as the _field exports, each the _guide export with one more argument.  The term is one more per-waypoint term
 * of the same routine, so it reaches everything that routine reaches: the three step kernels, adx_guide_cost and the guided
 * selection.  Callers and fixtures depend on this definition -- a change is a new version, never an edit.
 *
 *   cells    float32 [scene_rows][Gy][Gx], 2 <= Gx, Gy <= 256, row-major (x is the fast axis).  Row r of a launch reads scene
 *            r % scene_rows, like discs and planes.  Node [i][j] lies at (x_min + j * dx, y_min + i * dy) in the model's own units
 *            and this tick's ego frame.  The geometry is one per launch, not per scene, and does not move with h.
 *   scalars  x_min, y_min, inv_dx = fp32(1 / dx), inv_dy = fp32(1 / dy) (formed on the host) and weight, by value.
 *   term     of one waypoint (x, y), evaluated AFTER the discs and planes of v1 into the same J, gx, gy and active count (a guide
 *            without a field therefore accumulates exactly v1's bits).  fp32, no contraction, every operation rounded on its
 *            own, in this order:
 *              u = (x - x_min) * inv_dx;  v = (y - y_min) * inv_dy
 *              inside iff u >= 0 && u <= (float)(Gx-1) && v >= 0 && v <= (float)(Gy-1)            (a NaN is outside)
 *              j = min((int)u, Gx-2);  i = min((int)v, Gy-2);  fu = u - (float)j;  fv = v - (float)i
 *              c00 = cells[i][j];  c01 = cells[i][j+1];  c10 = cells[i+1][j];  c11 = cells[i+1][j+1]
 *              a = c01 - c00;  b = c11 - c10;  top = c00 + fu * a;  bot = c10 + fu * b;  dv = bot - top
 *              C = top + fv * dv;  active iff inside && C > 0
 *              du = a + fv * (b - a)
 *              J = J + weight * C;  gx = gx + (weight * du) * inv_dx;  gy = gy + (weight * dv) * inv_dy
 *            (du, dv) / (dx, dy) is the exact gradient of the bilinear interpolant inside a cell.  Outside the raster the term is
 *            inactive: a caller who wants "off the map is forbidden" adds planes.  Negative and zero cells are legal; the term is
 *            inactive wherever the interpolant is not positive.  An active field term counts 1 in `active`.
 *   the rest everything else is v1, word for word: the per-step loop (lambda, cap, clip, moved), the partner recomputation, the
 *            order of the step, the wave butterfly of the cost, and the selection's violation, active, free and blocked.
 *   guide    the adx_guide beside the field may be NULL for adx_guide_cost_field and adx_traj_select_guide_field: no discs and no
 *            planes.  A step reads iters, lambda and cap from it: the step exports refuse a field without a guide.  A guide
 *            without tensors (n_discs == n_planes == 0) fits any field; one with tensors must hold the field's scene_rows.
 *            adx_traj_select_guide_field: the field's scene_rows equals `scenes`.
 *   NULL     a NULL field is exactly the _guide export.
 *
 * ADX_ERR_INVALID before any GPU work, each with its own text: NULL cells; gx or gy outside 2..256; scene_rows < 1 or not
 * dividing batch; scene_rows disagreeing with the guide's when both hold tensors; inv_dx or inv_dy not finite or not > 0; weight
 * NaN or negative; x_min or y_min not finite; an output overlapping cells; a step with a field and no guide; and whatever the
 * _guide export refuses.
 * -----------------------------------------------------------------------------------*/
#define ADX_FIELD_MIN_NODES 2
#define ADX_FIELD_MAX_NODES 256
typedef struct adx_guide_field {
  const float* cells;          /* [scene_rows][gy][gx] */
  int32_t scene_rows, gx, gy;
  float x_min, y_min, inv_dx, inv_dy, weight;
} adx_guide_field;
int adx_ddim_step_field(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                        const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                        const adx_guide_field* field, float* prev, float* x0, int32_t batch, int32_t horizon, int32_t dim,
                        adx_stream s);
int adx_ddpm_step_field(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                        const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                        const adx_guide_field* field, float* prev, float* x0, int32_t batch, int32_t horizon, int32_t dim,
                        adx_stream s);
int adx_dpm_step_field(const adx_dpm_coef* c, const float* model_output, const float* sample, const float* prev_x0,
                       const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                       const adx_guide_field* field, float* prev_sample, float* x0, int32_t batch, int32_t horizon, int32_t dim,
                       adx_stream s);
int adx_guide_cost_field(const float* traj, const adx_guide* guide, const adx_guide_field* field, float* cost, int32_t* active,
                         int32_t rows, int32_t horizon, int32_t dim, adx_stream s);
int adx_traj_select_guide_field(const adx_select_guide_cfg* c, const float* trajs, const float* target, const adx_guide* guide,
                                const adx_guide_field* field, float* cost, int32_t* active, int32_t* index, int32_t* blocked,
                                float* best, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Cost guidance v3: cost guidance v2 plus MOTION LIMITS -- how fast to go.  For this model speed is the spacing of the
 * waypoints (the controller derives its desired speed from the mean segment length), so a per-scene cap on the length of a
 * segment is a speed limit and a cap on the length of a second difference is an acceleration limit.  v1 and v2 stay as they are:
 * the _guide and _field exports and their bits; v3 stands beside them as the _motion exports, each the _field export with one
 * more argument.  These are the first terms that couple a waypoint to its neighbours.  Callers and fixtures depend on this
 * definition -- a change is a new version, never an edit.
 *
 *   limits   float32 [scene_rows][2] = (s_max, a_max) in device memory, read at every launch.  Row r of a launch reads scene
 *            r % scene_rows.  Units are the model's own (the clamped result BEFORE xy scaling), per waypoint interval: s_max caps
 *            |p[i+1] - p[i]|, a_max caps |p[i+1] - 2 p[i] + p[i-1]|.  +inf switches a term off for that scene; so does a NaN,
 *            because every comparison with it is false.  s_max = 0 is legal: "do not move".
 *   weights  w_speed and w_accel, host scalars by value, >= 0.  A weight of exactly 0: the term is not evaluated and counts
 *            nothing in `active`.
 *   terms    of a row p[0..H-1], p[i] = (x, y) of waypoint i.  fp32, no contraction, every operation rounded on its own, in this
 *            order; S2 = s_max * s_max and A2 = a_max * a_max (one rounded product each, formed in the kernel):
 *              segment i, 0 <= i <= H-2:
 *                ex = x[i+1] - x[i];  ey = y[i+1] - y[i];  s2 = ex * ex + ey * ey;  phi = s2 - S2;  active iff phi > 0
 *                cost  (w_speed * (phi * phi)) / 2;   k = w_speed * (2 * phi)
 *                d/dp[i+1] = +(k * ex, k * ey);   d/dp[i] = -(k * ex, k * ey)
 *              curvature i, 1 <= i <= H-2:
 *                cx = (x[i+1] - x[i]) - (x[i] - x[i-1]);  cy likewise;  a2 = cx * cx + cy * cy;  psi = a2 - A2;  active iff psi > 0
 *                cost  (w_accel * (psi * psi)) / 2;   q = w_accel * (2 * psi)
 *                d/dp[i-1] = +(q * cx, q * cy);   d/dp[i] = -((2 * q) * cx, (2 * q) * cy);   d/dp[i+1] = +(q * cx, q * cy)
 *            No square root and no singular point.  H = 1 has no term, H = 2 one segment and no curvature.
 *   share    of waypoint h, evaluated AFTER v1's discs and planes and v2's field term into the same J, gx, gy and active count:
 *              J and active:  segment h-1 (h >= 1), then curvature h (1 <= h <= H-2): J = J + cost, active = active + 1
 *              gx, gy:        segment h-1 (+k e), segment h (-k e), curvature h-1 (+q c), curvature h (-(2 q) c),
 *                             curvature h+1 (+q c), in this order, each as g = g + t or g = g - t with t the rounded product
 *            A term that does not exist at that h is not added, and neither is an inactive one -- not even as a zero: a guide
 *            whose motion terms are all inactive accumulates exactly v2's bits.  Every waypoint that touches a term evaluates it
 *            anew from the same operands, so all agree on its bits.  Summed over a row, J counts every term once.
 *   anchor   the motion terms' gradient at h = 0 is not applied: the ego's present pose is not moved to satisfy a limit on its
 *            future.  Waypoint 0 still takes the v1 and v2 gradient, and segment 0 and curvature 1 read it as the value it has.
 *   per step the iterations of v1 become Jacobi iterations of the whole row.  From p = the step's clipped pred_original_sample
 *            of every waypoint; for it = 0..iters-1: every waypoint's g = the total gradient (v1, v2, v3) on iterate `it` of the
 *            whole row; then every waypoint moves, p = p - clamp(lambda * g, -cap, +cap), followed by the step's clip.  iters,
 *            lambda, cap, `moved` and everything after the guide are v1's, word for word: DDIM re-derives eps, DDPM and DPM
 *            read x0, the x0 output is the guided value, and an element that did not move runs the unguided step bit for bit.
 *   kernels  a wave owns a row (lane = waypoint), which needs horizon <= 64.  A step with a motion record always runs the
 *            row-wise kernel, whatever the weights and limits; with both weights 0, or every limit +inf, its results are the
 *            _field export's bit for bit.
 *   cost     adx_guide_cost_motion: per waypoint J as above, summed by v1's butterfly.  adx_traj_select_guide_motion: violation,
 *            active, free and blocked of selection cost v2 with these terms among them; the limits' scene_rows equals `scenes`.
 *            `hard` inherits v1's property: a candidate one ulp over a limit is not free.
 *   NULL     a NULL motion record is exactly the _field export (and the element-wise kernels).
 *
 * ADX_ERR_INVALID before any GPU work, each with its own text: NULL limits; scene_rows < 1 or not dividing batch; scene_rows
 * disagreeing with the guide's (when it holds discs or planes) or with the field's; a weight negative or NaN; horizon > 64; an
 * output overlapping limits; a step with motion limits and no adx_guide; and whatever the _field export refuses.
 * -----------------------------------------------------------------------------------*/
typedef struct adx_guide_motion {
  const float* limits;         /* [scene_rows][2] = (s_max, a_max) */
  int32_t scene_rows;
  float w_speed, w_accel;
} adx_guide_motion;
int adx_ddim_step_motion(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                         const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                         const adx_guide_field* field, const adx_guide_motion* motion, float* prev, float* x0, int32_t batch,
                         int32_t horizon, int32_t dim, adx_stream s);
int adx_ddpm_step_motion(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                         const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                         const adx_guide_field* field, const adx_guide_motion* motion, float* prev, float* x0, int32_t batch,
                         int32_t horizon, int32_t dim, adx_stream s);
int adx_dpm_step_motion(const adx_dpm_coef* c, const float* model_output, const float* sample, const float* prev_x0,
                        const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                        const adx_guide_field* field, const adx_guide_motion* motion, float* prev_sample, float* x0, int32_t batch,
                        int32_t horizon, int32_t dim, adx_stream s);
int adx_guide_cost_motion(const float* traj, const adx_guide* guide, const adx_guide_field* field, const adx_guide_motion* motion,
                          float* cost, int32_t* active, int32_t rows, int32_t horizon, int32_t dim, adx_stream s);
int adx_traj_select_guide_motion(const adx_select_guide_cfg* c, const float* trajs, const float* target, const adx_guide* guide,
                                 const adx_guide_field* field, const adx_guide_motion* motion, float* cost, int32_t* active,
                                 int32_t* index, int32_t* blocked, float* best, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Cost guidance v4: cost guidance v3 plus a ROUTE CORRIDOR -- where the road is.  v1 to v3 say where not to go and how fast; the
 * route is a per-scene polyline and a half-width, and a waypoint further than the half-width from the polyline pays for it and
 * is pulled back.  v1, v2 and v3 stay as they are: the _guide, _field and _motion exports, their structs and their bits; v4 stands
 * beside them as the _route exports, each the _motion export with one more argument.  The term is point-wise and couples no
 * neighbours, so it is one more term of the routine every guided kernel calls and reaches all of them: the element-wise step
 * kernels (no limits), the row-wise ones (limits), adx_guide_cost and the guided selection, which agree on its bits.  Callers and
 * fixtures depend on this definition -- a change is a new version, never an edit.
 *
 * Everything is in the model's own units (the clamped result BEFORE xy scaling) and this tick's ego frame, as in v1.
 *
 *   points      float32 [scene_rows][R][2] = (x, y) in device memory, 2 <= R <= 32 (ADX_ROUTE_MAX_POINTS), read at every launch.
 *               Segment i joins point i and point i+1, 0 <= i <= R-2.  Row r of a launch reads scene r % scene_rows.  Scenes with
 *               fewer points pad by repeating their last point: a degenerate segment is a legal segment, the point itself
 *               (t = 0, r = u).  Where that point is the nearest of the route, a padding segment's residual p - b may beat the last
 *               real segment's (p - a) - (b - a) by a rounding; nowhere else does padding change a bit.
 *   half_width  float32 [scene_rows] in device memory, read at every launch.  W2 = w * w, one rounded product, formed in the
 *               kernel.  +inf switches the term off for that scene; so does a NaN, because every comparison with it is false.
 *               0 is legal: "pull onto the route".
 *   weight      a host scalar by value, >= 0.  At exactly 0 the term is not evaluated and counts nothing in `active`.
 *   term        of one waypoint (x, y), evaluated AFTER v2's field term and BEFORE v3's motion terms into the same J, gx, gy and
 *               active count.  fp32, no contraction, every operation rounded on its own, in this order (px[i], py[i] are the
 *               points'):
 *                 best = +inf;  qx = qy = 0
 *                 for i = 0 .. R-2, in index order:
 *                   ax = px[i];  ay = py[i];  ex = px[i+1] - ax;  ey = py[i+1] - ay
 *                   ux = x - ax;  uy = y - ay
 *                   ee = ex * ex + ey * ey;  ue = ux * ex + uy * ey
 *                   t  = ee > 0 ? ue / ee : 0;   t = t < 0 ? 0 : (t > 1 ? 1 : t)            (a NaN passes through)
 *                   rx = ux - t * ex;  ry = uy - t * ey;  d2 = rx * rx + ry * ry
 *                   if d2 < best: best = d2; qx = rx; qy = ry       (strict: the first of equals wins; a NaN never wins)
 *                 phi = best - W2;   active iff best < +inf and phi > 0
 *                 J = J + (weight * (phi * phi)) / 2;   k = weight * (2 * phi)
 *                 gx = gx + k * qx;   gy = gy + k * qy;   active = active + 1
 *               No square root.  The gradient is exact (d best / dp = 2 q) except on the medial axis, where it is the first
 *               winner's.  An inactive term adds nothing, not even a zero: a guide whose route term is off (weight 0, every
 *               width +inf) accumulates exactly the bits of v3 (or v2, or v1).
 *   the rest    iters, lambda, cap, `moved`, the order inside a step and everything after the guide are v1's (or v3's, with
 *               limits), word for word.  In the element-wise kernels the x and the y thread of a waypoint each repeat its
 *               iterations, as in v1, so the term is evaluated twice per waypoint there.
 *   kernels     `field` and `motion` may each be NULL.  A NULL motion runs the element-wise kernels, a non-NULL one the row-wise
 *               ones (and needs horizon <= 64, as in v3).  No kernel is added: the guided kernels branch on points != NULL, which
 *               is the same in every thread of a launch.
 *   cost        adx_guide_cost_route: per waypoint J as above, summed by v1's butterfly.  adx_traj_select_guide_route: violation,
 *               active, free and blocked of selection cost v2 carry the route term among the others; the route's scene_rows
 *               equals `scenes`.  With `hard`, a candidate that leaves the corridor -- by one ulp of best - W2 -- is "not free".
 *   NULL        a NULL route is exactly the _motion export.
 *
 * ADX_ERR_INVALID before any GPU work, each with its own text: NULL points or half_width; n_points outside 2..32; scene_rows < 1
 * or not dividing batch; scene_rows disagreeing with the guide's (when it holds discs or planes), the field's or the limits'; a
 * weight negative or NaN; an output overlapping points or half_width; a step with a route and no adx_guide; and whatever the
 * _motion export refuses.
 * -----------------------------------------------------------------------------------*/
#define ADX_ROUTE_MIN_POINTS 2
#define ADX_ROUTE_MAX_POINTS 32
typedef struct adx_guide_route {
  const float* points;         /* [scene_rows][n_points][2] = (x, y) */
  const float* half_width;     /* [scene_rows] */
  int32_t scene_rows, n_points;
  float weight;
} adx_guide_route;
int adx_ddim_step_route(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                        const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                        const adx_guide_field* field, const adx_guide_motion* motion, const adx_guide_route* route, float* prev,
                        float* x0, int32_t batch, int32_t horizon, int32_t dim, adx_stream s);
int adx_ddpm_step_route(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                        const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                        const adx_guide_field* field, const adx_guide_motion* motion, const adx_guide_route* route, float* prev,
                        float* x0, int32_t batch, int32_t horizon, int32_t dim, adx_stream s);
int adx_dpm_step_route(const adx_dpm_coef* c, const float* model_output, const float* sample, const float* prev_x0,
                       const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                       const adx_guide_field* field, const adx_guide_motion* motion, const adx_guide_route* route, float* prev_sample,
                       float* x0, int32_t batch, int32_t horizon, int32_t dim, adx_stream s);
int adx_guide_cost_route(const float* traj, const adx_guide* guide, const adx_guide_field* field, const adx_guide_motion* motion,
                         const adx_guide_route* route, float* cost, int32_t* active, int32_t rows, int32_t horizon, int32_t dim,
                         adx_stream s);
int adx_traj_select_guide_route(const adx_select_guide_cfg* c, const float* trajs, const float* target, const adx_guide* guide,
                                const adx_guide_field* field, const adx_guide_motion* motion, const adx_guide_route* route,
                                float* cost, int32_t* active, int32_t* index, int32_t* blocked, float* best, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Cost guidance v5: cost guidance v4 plus MOVING CAPSULES -- the other road users as what they are.  v1's moving obstacles are
 * discs; a 4.5 m x 2 m car is not one.  A capsule is a segment with a radius, moving at a constant velocity: its distance is the
 * point-to-segment distance of v4, its potential exactly v1's disc potential around the nearest point of the segment, so a disc is
 * the capsule of zero length.  v1 to v4 stay as they are: the _guide, _field, _motion and _route exports, their structs and their
 * bits; v5 stands beside them as the _capsule exports, each the _route export with one more argument.  The term is point-wise and
 * couples no neighbours, so it is one more term of the routine every guided kernel calls and reaches all of them: the element-wise
 * step kernels (no limits), the row-wise ones (limits), adx_guide_cost and the guided selection, which agree on its bits.  Callers
 * and fixtures depend on this definition -- a change is a new version, never an edit.
 *
 * Everything is in the model's own units (the clamped result BEFORE xy scaling) and this tick's ego frame, as in v1.
 *
 *   capsules    float32 [scene_rows][C][7] = (ax, ay, bx, by, vx, vy, r) in device memory, 1 <= C <= 32 (ADX_CAPSULE_MAX), read at
 *               every launch.  Row r of a launch reads scene r % scene_rows.  (ax, ay) and (bx, by) are the ends of the axis at
 *               waypoint 0; at waypoint h both have moved by h * (vx, vy), v1's constant-velocity model.  A slot with r <= 0 or
 *               a NaN r is empty.  a == b is legal: a disc.
 *   weight      a host scalar by value, >= 0.  At exactly 0 the term is not evaluated and counts nothing in `active`.
 *   term        of one waypoint (x, y) at index h (hf = (float)h), evaluated AFTER v4's route term and BEFORE v3's motion terms
 *               into the same J, gx, gy and active count.  fp32, no contraction, every operation rounded on its own, in this
 *               order, for i = 0 .. C-1 in index order (q = capsules[scene][i]):
 *                 r = q[6];  skip unless r > 0
 *                 hx = hf * vx;  hy = hf * vy;  px = ax + hx;  py = ay + hy
 *                 ex = bx - ax;  ey = by - ay                      (from the unmoved ends: both move alike)
 *                 ux = x - px;   uy = y - py
 *                 ee = ex * ex + ey * ey;   ue = ux * ex + uy * ey
 *                 t  = ee > 0 ? ue / ee : 0;   t = t < 0 ? 0 : (t > 1 ? 1 : t)            (a NaN passes through)
 *                 rx = ux - t * ex;  ry = uy - t * ey;  d2 = rx * rx + ry * ry
 *                 rr = r * r;  inv = 1 / rr;  sd = d2 * inv;  phi = 1 - sd;   active iff phi > 0
 *                 J  = J + (weight * (phi * phi)) / 2
 *                 k  = weight * ((2 * phi) * inv)
 *                 gx = gx - k * rx;  gy = gy - k * ry;  active = active + 1
 *               No square root.  The potential is v1's: 1/2 on the axis, falling to 0 at distance r from it, so the capsule is
 *               the set of points within r of the segment.  The gradient is exact off the axis (d d2 / dp = 2 (rx, ry), also
 *               where t is clamped); ON the axis it is zero, as at a disc's centre: a waypoint exactly there is not pushed.
 *               An inactive or empty slot adds nothing, not even a zero: a guide whose capsule term is off (weight 0, every
 *               radius 0 or NaN) accumulates exactly the bits of v4 (or v3, v2, v1).  A capsule with a == b at weight 1
 *               accumulates exactly the bits of v1's disc (ax, ay, vx, vy, r): ee = 0, t = 0, (rx, ry) = (ux, uy).  A NaN in
 *               a slot's ends or velocity stays in that slot: phi is NaN and the slot is inactive.
 *   the rest    iters, lambda, cap, `moved`, the order inside a step and everything after the guide are v1's (or v3's, with
 *               limits), word for word.  In the element-wise kernels the x and the y thread of a waypoint each repeat its
 *               iterations, as in v1 and v4, so the term is evaluated twice per waypoint there; the row-wise kernels evaluate it
 *               once per lane.
 *   kernels     `field`, `motion` and `route` may each be NULL.  A NULL motion runs the element-wise kernels, a non-NULL one the
 *               row-wise ones (and needs horizon <= 64, as in v3).  No kernel is added: the guided kernels branch on
 *               capsules != NULL, which is the same in every thread of a launch.  The slots are read from global memory as they
 *               lie: a scene's capsules are at most 896 bytes that every lane of the scene reads at the same addresses.
 *   cost        adx_guide_cost_capsule: per waypoint J as above, summed by v1's butterfly.  adx_traj_select_guide_capsule:
 *               violation, active, free and blocked of selection cost v2 carry the capsule term among the others; the capsules'
 *               scene_rows equals `scenes`.  With `hard`, a candidate inside a capsule -- by one ulp of phi -- is "not free".
 *   NULL        NULL capsules are exactly the _route export.
 *
 * ADX_ERR_INVALID before any GPU work, each with its own text: NULL capsules data; n_capsules outside 1..32; scene_rows < 1 or
 * not dividing batch; scene_rows disagreeing with the guide's (when it holds discs or planes), the field's, the limits' or the
 * route's; a weight negative or NaN; an output overlapping the capsules; a step with capsules and no adx_guide; and whatever the
 * _route export refuses.
 * -----------------------------------------------------------------------------------*/
#define ADX_CAPSULE_MAX 32
typedef struct adx_guide_capsules {
  const float* capsules;       /* [scene_rows][n_capsules][7] = (ax, ay, bx, by, vx, vy, r) */
  int32_t scene_rows, n_capsules;
  float weight;
} adx_guide_capsules;
int adx_ddim_step_capsule(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                          const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                          const adx_guide_field* field, const adx_guide_motion* motion, const adx_guide_route* route,
                          const adx_guide_capsules* capsules, float* prev, float* x0, int32_t batch, int32_t horizon, int32_t dim,
                          adx_stream s);
int adx_ddpm_step_capsule(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                          const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                          const adx_guide_field* field, const adx_guide_motion* motion, const adx_guide_route* route,
                          const adx_guide_capsules* capsules, float* prev, float* x0, int32_t batch, int32_t horizon, int32_t dim,
                          adx_stream s);
int adx_dpm_step_capsule(const adx_dpm_coef* c, const float* model_output, const float* sample, const float* prev_x0,
                         const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                         const adx_guide_field* field, const adx_guide_motion* motion, const adx_guide_route* route,
                         const adx_guide_capsules* capsules, float* prev_sample, float* x0, int32_t batch, int32_t horizon,
                         int32_t dim, adx_stream s);
int adx_guide_cost_capsule(const float* traj, const adx_guide* guide, const adx_guide_field* field, const adx_guide_motion* motion,
                           const adx_guide_route* route, const adx_guide_capsules* capsules, float* cost, int32_t* active,
                           int32_t rows, int32_t horizon, int32_t dim, adx_stream s);
int adx_traj_select_guide_capsule(const adx_select_guide_cfg* c, const float* trajs, const float* target, const adx_guide* guide,
                                  const adx_guide_field* field, const adx_guide_motion* motion, const adx_guide_route* route,
                                  const adx_guide_capsules* capsules, float* cost, int32_t* active, int32_t* index, int32_t* blocked,
                                  float* best, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Trajectory modes v1: which different manoeuvres a scene's K candidates contain, and how many candidates back each one.  The
 * candidates are clustered by a greedy cover under a radius, in one launch with no host decision (a node of a captured graph).
 * No reference counterpart: the reference's train.evaluate draws many trajectories for one image only to paint them
 * (train.py:62-90).  Callers and fixtures depend on this definition -- a change is a new version, never an edit.
 *
 *   layout   trajs [candidates * scenes][H][D], CANDIDATE-MAJOR as adx_traj_select takes them: candidate k of scene s is row
 *            k * scenes + s.  modes [max_modes * scenes][H][D], MODE-MAJOR in the same way: mode m of scene s is row
 *            m * scenes + s, so that the tensor is an M-candidate set to adx_traj_select, adx_traj_metrics and adx_guide_cost as
 *            it is.  index and mass int32 [scenes][max_modes]; assign int32 [scenes][candidates]; count int32 [scenes]; dist2
 *            float32 [scenes][candidates][candidates] or NULL (not written).  With K = candidates, M = max_modes, S = scenes:
 *   points   p_h = (x, y) = the first min(D, 2) columns of waypoint h; a missing y column (D = 1) counts as 0.  Only the waypoints
 *            h0 <= h <= H-1 are scored, n = H - h0 of them (callers pass h0 = 1: waypoint 0 is the ego pose the sampling loops
 *            zero).  Units are those of trajs.
 *   finite   candidate k is finite when every scored x and y of it is finite.  Columns >= 2 and waypoints below h0 are never read
 *            for a decision (only copied, by `modes`).
 *   dist2    dist2[i][j] = the mean over the scored h of |p_i,h - p_j,h|^2, in fp32: per h, dx = x_i - x_j, dy = y_i - y_j,
 *            t_h = dx * dx + dy * dy; the t_h are added one by one in the order h = h0, h0 + 1, .. H-1, starting from t_h0, and the
 *            sum is divided by (float)n.  Every product, sum and the division is rounded on its own (no contraction).  So
 *            dist2[i][j] and dist2[j][i] hold the same bits and dist2[i][i] is 0 for a finite i.  Entries that involve a
 *            non-finite candidate are unspecified and enter no decision.
 *   near     i and j are near when both are finite and dist2[i][j] <= r2, r2 = radius * radius rounded once in fp32.  A finite
 *            candidate is near itself.
 *   greedy cover  alive = the finite candidates.  For m = 0 .. M-1, while alive is not empty: for every alive i, n_i = the number
 *            of alive j (i included) near i; rep = the smallest i with the largest n_i; index[m] = rep, mass[m] = n_rep; every
 *            alive j near rep gets assign[j] = m and leaves alive.  count[s] = the number of modes formed.  The masses are
 *            non-increasing by construction (what is alive only shrinks).
 *   the rest candidates still alive after M modes are outliers: assign = -1.  Non-finite candidates: assign = -2.  Slots
 *            m >= count: index = -1, mass = 0.
 *   modes    for m < count, row m * S + s of modes is row index[m] * S + s of trajs, all H * D values bit for bit.  For
 *            m >= count it is a copy of mode 0's row (a downstream min over the M rows is then never won by a filler); when
 *            count = 0 (no finite candidate) all M rows are zeros.
 *   arithmetic  no atomics and no traffic between workgroups, fixed orders everywhere: the same input gives the same bits on
 *            every launch, and a scene's result does not depend on the other scenes of the launch.  dist2 is defined up to fp32
 *            rounding of the operations above (tests/modes_ref.py restates it in fp64 and derives the bound); every integer
 *            output and modes exactly wherever no |dist2[i][j] - r2| of a finite pair lies within that rounding.
 *
 * Limits: 1 <= candidates <= 64, 1 <= max_modes <= 64, 1 <= horizon <= 64, 1 <= dim <= 16, 1 <= scenes <= 65535,
 * 0 <= h0 <= horizon - 1, radius finite and >= 0.  ADX_ERR_INVALID before any GPU work, each with its own text, for a value out of
 * range, a NULL pointer other than dist2, or an output that overlaps trajs or another output.
 * -----------------------------------------------------------------------------------*/
typedef struct adx_modes_cfg {
  int32_t scenes, candidates, horizon, dim, max_modes, h0;
  float radius;
} adx_modes_cfg;
int adx_traj_modes(const adx_modes_cfg* c, const float* trajs, float* modes, int32_t* index, int32_t* mass, int32_t* assign,
                   int32_t* count, float* dist2 /* or NULL */, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Manoeuvre commitment v1: hold the manoeuvre the previous tick chose unless the selector's new choice is clearly better.  A
 * selector that takes the arg-min of a cost over fresh samples changes its mind on sampling noise alone wherever two manoeuvres
 * cost nearly the same; this node, one launch between selection and everything that consumes the winner, compares the K
 * candidates with the plan the last tick chose (moved on by the odometry) and keeps the cheapest candidate near that plan while
 * the selector's own is not better by a threshold.  Everything it needs is on the device and it advances its own state there: no
 * host decision, the same node on the first tick and on every later one (a node of a captured graph).  No reference counterpart:
 * the reference samples one trajectory per tick (interact.py:110-140).  Callers and fixtures depend on this definition -- a change
 * is a new version, never an edit.
 *
 *   layout   trajs [candidates * scenes][H][D], CANDIDATE-MAJOR exactly as adx_traj_select takes them (candidate k of scene s is
 *            row k * scenes + s): the clamped, unscaled candidates.  cost float32 [scenes][candidates] and selected int32 [scenes]:
 *            the selector's cost and index outputs.  active int32 [scenes][candidates]: the guided selector's violation counts, or
 *            NULL.  motion float32 [scenes][3] = (tx, ty, phi) with warm start v1's meaning, or NULL.  best [scenes][H][D]; index,
 *            status, follower int32 [scenes]; blocked int32 [scenes] or NULL; dist2 float32 [scenes][candidates].  With
 *            K = candidates, S = scenes:
 *   state    one device buffer of adx_commit_state_bytes(scenes, horizon) bytes: 32-bit words [scenes][2 + 2H].  Word 0: `valid`,
 *            int32.  Word 1: `held`, int32, the consecutive ticks the node has overridden the selector.  Words 2 + 2h and 3 + 2h:
 *            x and y (float32) of waypoint h of the plan chosen on the last tick, in that tick's frame.  All zero bytes = fresh.
 *            Every launch reads and advances the state through its address -- nothing about it is a by-value argument -- so a
 *            captured graph carries it from replay to replay, the first tick included.  A scene's state is read completely
 *            before any word of it is written.
 *   prior    for valid != 0: q_h, h = 0 .. H-1, is warm start v1's `advance` followed by its `re-base`, applied to the stored
 *            [H][2] plan (columns 0 and 1 alone) with this launch's `shift` and `motion`: the same operations in the same order,
 *            every one rounded on its own (no contraction); without motion the origin is the stored waypoint `shift`.  It is not
 *            clamped and draws no noise.  With motion, cos(phi) and sin(phi) are the device library's cosf and sinf.  The prior is
 *            ABSENT when valid == 0 or any scored q_h (below) has a non-finite x or y.
 *   points   p_k,h = (x, y) = the first min(D, 2) columns of waypoint h of candidate k; a missing y column (D = 1) counts as 0.
 *            Only the waypoints h0 <= h <= H-1 are scored, n = H - h0 of them.
 *   dist2    d_k = the mean over the scored h of |p_k,h - q_h|^2 in trajectory modes v1's arithmetic: per h, dx = x_k - qx,
 *            dy = y_k - qy, t_h = dx * dx + dy * dy; the t_h are added one by one in the order h = h0 .. H-1 starting from t_h0,
 *            and the sum is divided by (float)n; every operation rounded on its own.  dist2[s][k] = d_k.  Entries of non-finite
 *            candidates are unspecified; all of dist2 is unspecified when the prior is absent.
 *   finite   candidate k is finite when every scored x and y of it is finite.
 *   near     k is near when it is finite and d_k <= r2, r2 = radius * radius rounded once in fp32.
 *   eligible k is eligible when it is near, cost[k] is finite, and (active is NULL, or active[k] == 0, or active[sel] != 0): a
 *            violating follower never replaces a free winner.
 *   decision with sel = selected[s] (a value outside 0..K-1 cannot be refused on the host: the kernel CLAMPS it into range), the
 *            first rule that matches:
 *              status 0  NO_PRIOR   the prior is absent                                              chosen = sel
 *              status 1  SAME       sel is near                                                      chosen = sel
 *              status 2  LOST       no candidate is eligible                                         chosen = sel
 *              status 3  HELD       f = the eligible candidate of smallest cost (ties: the lowest index); cost[f] <= t with
 *                                   t = (cost[sel] + margin) + ratio * fabsf(cost[sel]), every operation rounded on its own; and
 *                                   max_hold == 0 or held < max_hold                                 chosen = f
 *              status 4  SWITCHED   otherwise                                                        chosen = sel
 *            A NaN in any comparison makes it false.  follower[s] = f, or -1 where no f was formed (statuses 0, 1, 2).
 *   outputs  best[s] = row chosen * S + s of trajs, all H * D words bit for bit; index[s] = chosen; status[s]; follower[s];
 *            blocked[s] = (active[chosen] != 0), written only when both active and blocked are given.
 *   update   held' = held + 1 on HELD, otherwise 0.  When the chosen candidate is finite: valid' = 1 and the stored x and y become
 *            its columns 0 and 1 of ALL H waypoints (y = 0 when D = 1).  Otherwise valid' = 0 and the stored plan keeps its words.
 *   arithmetic  no atomics and no traffic between workgroups, fixed orders everywhere: the same input and state give the same bits
 *            on every launch, and a scene's result does not depend on the other scenes of the launch.  Without motion nothing
 *            above is transcendental and every output and the next state are defined to the bit (tests/commit_ref.py restates
 *            them in fp32); with motion dist2 is defined up to the rounding tests/commit_ref.py derives (dist2_bound), and the
 *            decisions exactly wherever no finite candidate's |d_k - r2| lies within it.
 *
 * adx_commit_reset zeroes the state of every scene (mask NULL) or of the scenes whose mask byte is not 0 (uint8 [scenes]): one
 * small capturable launch.  adx_commit_state_bytes is 0 for a value out of range.
 *
 * Limits: 1 <= candidates <= 64, 2 <= horizon <= 64 (advance reads waypoint H-2), 1 <= dim <= 16, 1 <= scenes <= 65535,
 * 0 <= h0 <= horizon - 1, 0 <= shift <= horizon - 1, max_hold >= 0, radius, margin and ratio finite and >= 0.  ADX_ERR_INVALID
 * before any GPU work, each with its own text, for a value out of range, a NULL pointer other than active, motion and blocked,
 * blocked given without active, an output that overlaps an input, the state or another output, or a state that overlaps an input.
 * -----------------------------------------------------------------------------------*/
typedef struct adx_commit_cfg {
  int32_t scenes, candidates, horizon, dim, h0, shift, max_hold;
  float radius, margin, ratio;
} adx_commit_cfg;
size_t adx_commit_state_bytes(int32_t scenes, int32_t horizon);
int adx_commit_reset(void* state, int32_t scenes, int32_t horizon, const uint8_t* mask /* or NULL: all */, adx_stream s);
int adx_traj_commit(const adx_commit_cfg* c, const float* trajs, const float* cost, const int32_t* selected,
                    const int32_t* active /* or NULL */, const float* motion /* or NULL */, void* state, float* best, int32_t* index,
                    int32_t* status, int32_t* follower, int32_t* blocked /* or NULL */, float* dist2, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Ego frame v1: the transform between world metres and a tick's ego frame in model units, the one the reference applies to its
 * target point (interact.py:185-202, process_next_waypoint) and undoes for its plans (interact.py:249-260, agent_to_world).  Both
 * launches below and route planner v1 evaluate exactly this.  Callers and fixtures depend on this definition -- a change is a new
 * version, never an edit.
 *
 *   pose     fp64 [scenes][3] = (px, py, compass) in device memory: world metres and radians.  A NaN compass counts as 0.
 *   frame    th = compass + pi/2 (pi/2 the double nearest to it), c = cos(th), s = sin(th): the device library's fp64 cos and sin.
 *   rotate   of a world vector (dx, dy), fp64, no contraction, every product and sum rounded on its own:
 *              r0 = c * dx + s * dy;   r1 = -(s * dx) + c * dy;   the ego vector is (r1, -r0)
 *            -- a proper rotation of the world by compass + pi, so lengths, angles and orientation are kept.
 *   point    of a world point (X, Y): dx = X - px, dy = Y - py, rotate, x = r1 / xy_scale, y = -r0 / xy_scale, each rounded to
 *            fp32 once.
 *   back     of an ego point (x, y) in model units (fp32, widened exactly): a0 = -(y * xy_scale), a1 = x * xy_scale,
 *            X = (c * a0 - s * a1) + px, Y = (s * a0 + c * a1) + py, fp64.
 *   rounding two evaluations of `point` that differ only in their cos and sin routines (each within 4 ulp) differ by at most one
 *            fp32 ulp of the result plus 8 * 2^-52 * (|dx| + |dy|) / xy_scale (tests/nav_ref.py derives the 8).
 *
 * adx_world_to_ego: one thread per record; `in` fp64 [scenes][n][w_in] world and physical, `out` fp32 [scenes][n][w_out] in the
 * formats the guide takes; vel_scale = dt / xy_scale, formed by the caller in fp64 (read by kinds 1 and 3 only):
 *   kind 0  points  (X, Y)                              -> (x, y)                               Route.points, target
 *   kind 1  discs   (cx, cy, vx, vy, r), m and m/s      -> (point(cx, cy), rotate(vx, vy) * vel_scale, r / xy_scale)
 *   kind 2  planes  (nx, ny, b): n . p <= b in world    -> (rotate(nx, ny), (b - (nx * px + ny * py)) / xy_scale)
 *   kind 3  boxes   (cx, cy, vx, vy, yaw, length, width); yaw the world angle of the heading
 *                                                       -> (point(cx, cy), rotate(vx, vy) * vel_scale, rotate(cos yaw, sin yaw),
 *                                                           length / xy_scale, width / xy_scale): adx_capsules_from_boxes's input
 *   A radius or size that is <= 0 or NaN is divided like any other and so stays <= 0 or NaN: an empty slot stays empty.
 *   Limits: 1 <= scenes <= 65535, 1 <= n <= 65536.
 *
 * adx_ego_to_world: plans fp32 [rows][horizon][dim] in model units, dim >= 2 (columns 0 and 1 are read), rows a positive multiple
 * of scenes; row r uses pose[r % scenes] (candidate-major rows).  out fp64 [rows][horizon][2] world metres by `back`.
 * Limits: 1 <= scenes <= 65535, 1 <= horizon <= 65536, 2 <= dim <= 16, rows * horizon <= 2^30.
 *
 * ADX_ERR_INVALID before any GPU work: a kind or a count out of range, a NULL pointer, xy_scale not finite and > 0, vel_scale not
 * finite (kinds 1 and 3), an output that overlaps an input.
 * -----------------------------------------------------------------------------------*/
#define ADX_EGO_POINTS 0
#define ADX_EGO_DISCS 1
#define ADX_EGO_PLANES 2
#define ADX_EGO_BOXES 3
int adx_world_to_ego(int32_t kind, const double* in, const double* pose, float* out, int32_t scenes, int32_t n, double xy_scale,
                     double vel_scale, adx_stream s);
int adx_ego_to_world(const float* plans, const double* pose, double* out, int32_t rows, int32_t scenes, int32_t horizon,
                     int32_t dim, double xy_scale, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Route planner v1: what feeds a tick, on the device -- the reference's RoutePlanner.run_step (e2e_driving/planner.py:55-92) for
 * every scene, its target point and the route ahead in this tick's ego frame, and the odometry between two ticks.  One launch, one
 * wave per scene, no host decision; the walk along the plan lives in a device buffer the launch reads and advances through its
 * address, so the call is capturable and the first tick is the same launch as every later one.  Callers and fixtures depend on
 * this definition -- a change is a new version, never an edit.
 *
 *   route    fp64 [scenes][G][2], world metres; cmd int32 [scenes][G]; len int32 [scenes]: the points a scene's plan holds.  len
 *            lives in device memory and cannot be refused on the host: the kernel CLAMPS it into 1..G.
 *   pose     fp64 [scenes][3] = (px, py, compass) as ego frame v1 takes it.
 *   state    one device buffer of adx_nav_state_bytes(scenes) = 32 * scenes bytes; per scene int32 `head`, int32 `valid`, then
 *            fp64 (px, py, compass) of the previous tick (the compass as used: a NaN stored as 0).  All zero bytes = a fresh walk
 *            from point 0.  `head` is the reference's deque as a cursor: the points before it are popped.  A stored head outside
 *            0..len-1 is clamped into it.  A scene's state is read completely before any word of it is written.
 *   walk     with n = len - head, pos = (px, py), all in fp64 without contraction:
 *              n == 1: next = head.
 *              otherwise cum = 0, far = -inf, to_pop = 0 and, for i = 1 .. n-1 in order: stop before i when cum > max_distance;
 *              cum = cum + |route[head+i] - route[head+i-1]|; d = |route[head+i] - pos|; when d <= min_distance and d > far:
 *              far = d, to_pop = i.  |v| = sqrt(v.x * v.x + v.y * v.y).  cum is the sequential sum in index order.  A NaN makes
 *              every comparison it enters false.  Then head += min(to_pop, max(n - 2, 0)) and next = head + 1.
 *   outputs  target fp32 [scenes][2] = point(route[next]); command int32 [scenes] = cmd[next], as stored;
 *            window fp32 [scenes][R][2]: point(route[min(head + first + k, len - 1)]), k = 0 .. R-1, with the NEW head: first = 1
 *            is the reference's get_future_waypoints (interact.py:174), first = 0 keeps the point just passed as well, so that a
 *            corridor covers the segment the ego is on; head_out int32 [scenes] = the new head.
 *   motion   fp32 [scenes][3] = (tx, ty, phi) with warm start v1's meaning, fresh int32 [scenes].  valid == 0: motion = 0 and
 *            fresh = 1.  Otherwise fresh = 0, (tx, ty) = `point` of this tick's position in the PREVIOUS pose's frame, and
 *            phi = d - 2 pi * ceil((d - pi) / (2 pi)) with d = compass - compass_prev: wrapped to (-pi, pi], then rounded to fp32.
 *            The ego frame is a proper rotation of the world by compass + pi, so a point q seen from the previous pose is
 *            R(-phi) (q - t) seen from this one: warm start v1's re-base.
 *   update   head, valid = 1 and this tick's pose (the compass as used).
 *
 * adx_nav_reset makes the walk of every scene (mask NULL) or of the scenes whose mask byte is not 0 (uint8 [scenes]) fresh: one
 * small capturable launch.  adx_nav_state_bytes is 0 for a value out of range.
 *
 * Limits: 1 <= scenes <= 65535, 1 <= max_points = G <= 65536, 2 <= window = R <= 32, first 0 or 1, min_distance, max_distance and
 * xy_scale finite and > 0.  ADX_ERR_INVALID before any GPU work, each with its own text, for a value out of range, a NULL
 * pointer, an output that overlaps an input, the state or another output, or a state that overlaps an input.
 * -----------------------------------------------------------------------------------*/
typedef struct adx_nav_cfg {
  int32_t scenes, max_points, window, first;
  double min_distance, max_distance, xy_scale;
} adx_nav_cfg;
size_t adx_nav_state_bytes(int32_t scenes);
int adx_nav_reset(void* state, int32_t scenes, const uint8_t* mask /* or NULL: all */, adx_stream s);
int adx_nav_step(const adx_nav_cfg* c, const double* route, const int32_t* cmd, const int32_t* len, const double* pose, void* state,
                 float* target, int32_t* command, float* window, float* motion, int32_t* fresh, int32_t* head_out, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Vehicle v1: a kinematic bicycle for every scene of a launch -- what takes a tick's (throttle, steer, brake) to the next pose, so
 * that a loop of ticks can be closed without a simulator.  One launch, one lane per scene, no host decision; the vehicle lives in a
 * device buffer the launch reads and advances through its address, so the call is capturable and the first step is the same launch
 * as every later one.  It is a model of a car, not of CARLA's: no tyres, no gears, no slopes.  Callers and fixtures depend on this
 * definition -- a change is a new version, never an edit.
 *
 *   state    one device buffer of adx_vehicle_state_bytes(scenes) = 40 * scenes bytes; per scene fp64 x, y, compass, speed, then
 *            int32 `valid` and one int32 of padding (kept 0).  All zero bytes = a vehicle at the origin, compass 0, at rest, not yet
 *            placed.  A scene's state is read completely before any word of it is written.
 *   control  fp32 [scenes][3] = (throttle, steer, brake) as control v1 writes it.  A component that is NaN or infinite counts as 0.
 *            Then throttle and brake are clamped into 0..1 and steer into -1..1 (control v1's throttle goes up to MAX_THROTTLE;
 *            a pedal does not), and all three are widened to fp64 exactly.
 *   hold     int32 [scenes] or NULL.  Where hold != 0 the scene stands still: speed = 0, yaw_rate = 0, x, y and compass kept,
 *            valid = 1; the control is not read.
 *   step     fp64, no contraction, every operation rounded on its own, in this order.  h = dt / substeps, formed on the host.
 *            delta = steer * steer_max;  k = tan(delta) / wheelbase  (the device library's fp64 tan; once per step).
 *            c0 = compass.  Then `substeps` times:
 *              a = throttle * accel_max - brake * brake_max - drag * v;   and a = a - roll when v > 0
 *                  (left to right: ((throttle * accel_max) - (brake * brake_max)) - (drag * v), then - roll)
 *              v = v + a * h;   v = 0 when v < 0 (or NaN);   v = v_max when v > v_max
 *              compass = compass + ((steer_sign * v) * k) * h           with the NEW v
 *              x = x + (v * h) * sin(compass);   y = y - (v * h) * cos(compass)       with the NEW compass
 *            (sin compass, -cos compass) is the world image of the ego +y unit vector under ego frame v1: `back` of (0, 1) with
 *            xy_scale 1 is (-cos(compass + pi/2), -sin(compass + pi/2)).  steer_sign = +1 turns the vehicle towards ego -x of ego
 *            frame v1 for a positive steer, which is what control v1 with sign_x = -1 asks for (tests/test_sim_cpu.py decides it).
 *            yaw_rate = (compass - c0) / dt.  The compass is not wrapped: ego frame v1 and route planner v1 take any angle.
 *   outputs  pose fp64 [scenes][3] = (x, y, compass): ego frame v1's and route planner v1's `pose`; velocity fp32 [scenes] = v and
 *            yaw_rate fp32 [scenes], each rounded to fp32 once: control v1's `velocity`.  Then the state = (x, y, compass, v, 1, 0).
 *   launch   64 lanes per workgroup, one lane per scene; every store to the state and to `pose` writes one 32-bit word per lane.
 *   rounding two evaluations that differ only in their tan, sin and cos routines (the device library's within 2 ulp -- an
 *            assumption: ROCm ships no accuracy table --, the host's within 1) differ per step by what tests/vehicle_ref.py derives.
 *
 * adx_vehicle_reset places vehicles: for every scene (mask NULL) or the scenes whose mask byte is not 0 (uint8 [scenes]) the state
 * becomes (pose[s], speed[s] or 0 when speed is NULL, valid = 1), a NaN compass or speed stored as 0 and a negative speed as 0;
 * with pose NULL the state becomes all zero (valid = 0).  The outputs pose, velocity and yaw_rate (= 0) of those scenes are
 * written as well when the three pointers are given (all or none), so a navigator can read the start pose.  One small capturable
 * launch.  adx_vehicle_state_bytes is 0 for a value out of range.
 *
 * Limits: 1 <= scenes <= 65535, 1 <= substeps <= 16; dt, wheelbase, accel_max, brake_max, v_max finite and > 0; drag, roll finite
 * and >= 0; 0 < steer_max < 1.5 (radians: below pi/2, where tan has its pole); steer_sign +1 or -1.  ADX_ERR_INVALID before any
 * GPU work, each with its own text, for a value out of range, a NULL pointer, an output that overlaps an input, the state or
 * another output, or a state that overlaps an input.
 * -----------------------------------------------------------------------------------*/
typedef struct adx_vehicle_cfg {
  int32_t scenes, substeps, steer_sign, reserved /* 0 */;
  double dt, wheelbase, accel_max, brake_max, drag, roll, v_max, steer_max;
} adx_vehicle_cfg;
size_t adx_vehicle_state_bytes(int32_t scenes);
int adx_vehicle_reset(void* state, int32_t scenes, const double* pose /* or NULL: zeros, not placed */,
                      const double* speed /* or NULL: 0 */, const uint8_t* mask /* or NULL: all */, double* pose_out /* or NULL */,
                      float* velocity_out /* or NULL */, float* yaw_rate_out /* or NULL */, adx_stream s);
int adx_vehicle_step(const adx_vehicle_cfg* c, const float* control, const int32_t* hold /* or NULL */, void* state, double* pose,
                     float* velocity, float* yaw_rate, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Drive metrics v1: the closed-loop criteria of a drive, advanced by one tick for every scene in one launch -- route completion,
 * cross-track error, collisions, route deviation, a stall clock, comfort, the odometer -- with every record in device memory and
 * one read at the end.  What the reference takes from CARLA's criteria (carla_gym/core/task_actor/common/criteria: RouteDeviation
 * and Blocked are restated; collisions are geometric because there is no physics engine to report them).  One wave per scene, no
 * host decision, capturable.  Callers and fixtures depend on this definition -- a change is a new version, never an edit.
 *
 *   inputs   pose fp64 [scenes][3], velocity fp32 [scenes], yaw_rate fp32 [scenes]: vehicle v1's outputs, or a simulator's or a
 *            log's.  A NaN compass counts as 0.  route fp64 [scenes][G][2] and len int32 [scenes] as route planner v1 takes them
 *            (len clamped into 1..G by the kernel); cum fp64 [scenes][G]: cum[0] = 0, cum[i] = cum[i-1] + |route[i] - route[i-1]|,
 *            summed sequentially by the caller; `length` = cum[len-1].  |v| = sqrt(v.x * v.x + v.y * v.y).
 *            discs fp64 [scenes][M][5] = (cx, cy, vx, vy, r) and boxes fp64 [scenes][N][7] = (cx, cy, vx, vy, yaw, length, width)
 *            in world metres AS OF THIS TICK (the velocities are not read), 0 <= M, N <= 64, NULL exactly when the count is 0.
 *            A radius or a size that is <= 0 or NaN marks an empty slot.
 *   state    adx_drive_state_bytes(scenes) = 192 * scenes bytes; per scene ten int32
 *              cursor, ticks, done, flags, contact, events, contact_ticks, first_tick, first_slot, have
 *            then nineteen fp64
 *              px, py, v_prev, a_prev, progress, progress_max, xtrack, xtrack_max, xtrack_sum, xtrack_sq, distance, offroad,
 *              stall, acc_max, acc_sq, jerk_max, jerk_sq, lat_max, lat_sq.
 *            All zero bytes = a drive not yet begun.  A scene whose `done` is not 0 is FROZEN: the launch writes done[s] again and
 *            nothing else of it.  Otherwise, in fp64 without contraction, with pos = (pose.x, pose.y):
 *   progress len == 1: j = 0, t = 0, d = |pos - route[0]|, progress = 0.  Otherwise the cursor is clamped into 0..len-2 and for
 *            every segment j in cursor .. min(cursor + window - 1, len - 2), a = route[j], u = route[j+1] - a, L2 = u.x * u.x +
 *            u.y * u.y:  t = 0 when not L2 > 0, else t = ((pos.x - a.x) * u.x + (pos.y - a.y) * u.y) / L2 clamped into 0..1 (a NaN
 *            becomes 0);  q = (a.x + t * u.x, a.y + t * u.y);  d = |pos - q|, a NaN d counting as +inf.  The winner is the smallest
 *            d, the LOWER j on a tie.  cursor = j;  progress = cum[j] + t * sqrt(L2);  progress_max = max(progress_max, progress);
 *            xtrack = d;  xtrack_max = max(xtrack_max, d), xtrack_sum += d, xtrack_sq += d * d.
 *   odometer step = |pos - (px, py)| when ticks > 0, else 0;  distance += step;  then (px, py) = pos.
 *   contact  the ego is n_discs discs of radius r_ego centred at pos + offset[k] * (sin compass, -cos compass), k < n_discs (the
 *            device library's fp64 sin and cos).  A live disc is hit when |centre - c| < r + r_ego for some k.  A live box is hit
 *            when the distance from a centre to the rectangle is < r_ego: e = centre - c, ux = cos yaw, uy = sin yaw,
 *            lx = e.x * ux + e.y * uy, ly = -(e.x * uy) + e.y * ux, qx = max(|lx| - length / 2, 0), qy = max(|ly| - width / 2, 0),
 *            |(qx, qy)| < r_ego.  hit = any slot hit.  events += hit and contact == 0 (a rising edge);  contact_ticks += hit;
 *            contact = hit.  On the first hit of a drive first_tick = the new `ticks` (so 1 is the first step; 0 = none yet) and
 *            first_slot = the lowest hit slot, disc j being slot j and box j slot 64 + j.
 *   deviate  the reference's RouteDeviation with xtrack as its distance: far = xtrack > offroad_max;  when xtrack > offroad_min:
 *            offroad += step, and share = offroad / length > max_route_percentage.  off = far or share.
 *   stall    the reference's Blocked as a clock: stall = velocity < speed_threshold ? stall + dt : 0;  blocked = stall > max_time.
 *            The reference keeps the time of the last valid state and reads the value 0.0 as "unset", so a vehicle that never
 *            moves after time 0 is never blocked; that quirk is NOT reproduced.
 *   comfort  v = velocity widened.  have >= 1: a = (v - v_prev) / dt, acc_max = max(acc_max, |a|), acc_sq += a * a.  have >= 2:
 *            jk = (a - a_prev) / dt, jerk_max, jerk_sq likewise.  lat = v * yaw_rate on every tick: lat_max, lat_sq.  Then
 *            v_prev = v, a_prev = a (when have >= 1), have = min(have + 1, 2).
 *   done     ticks += 1.  Then the FIRST of these that holds sets `done`, and `flags` gets bit (n - 1) of EVERY n that holds:
 *              1 completed   progress_max >= length - completion_tol
 *              2 collision   hit and stop_on_collision != 0
 *              3 off route   off
 *              4 blocked     blocked
 *              5 timeout     max_ticks > 0 and ticks >= max_ticks
 *            0 = running.  done int32 [scenes] is written on every launch: an output a vehicle's `hold` can point at.
 *   launch   one workgroup of one wave per scene.  Lanes take 64 segments at a time; one xor butterfly over (d, j) keeps the
 *            smaller d and the lower j on a tie, and a later chunk replaces the carried winner only with a strictly smaller d.
 *            Lane j tests disc j and box j; a ballot reduces the hit.  Lane 0 forms the record, lanes 0 .. 47 store one 32-bit
 *            word of it each.
 *
 * adx_drive_reset zeroes the records of every scene (mask NULL) or of the scenes whose mask byte is not 0, and their done[s] when
 * `done` is given: one small capturable launch.  adx_drive_state_bytes is 0 for a value out of range.
 *
 * Limits: 1 <= scenes <= 65535, 1 <= max_points = G <= 65536, 1 <= window <= 65536, 0 <= n_world_discs = M <= 64, 0 <= n_boxes = N
 * <= 64, 1 <= n_discs <= 4, max_ticks >= 0; dt finite and > 0; r_ego, offroad_min, offroad_max, max_route_percentage,
 * speed_threshold, max_time, completion_tol finite and >= 0; offsets finite.  ADX_ERR_INVALID before any GPU work, each with its own
 * text, for a value out of range, a NULL pointer (or discs / boxes not NULL exactly when their count is 0), an output that
 * overlaps an input, or a state that overlaps an input or `done`.
 * -----------------------------------------------------------------------------------*/
typedef struct adx_drive_cfg {
  int32_t scenes, max_points, window, n_world_discs, n_boxes, n_discs, stop_on_collision, max_ticks;
  double dt, r_ego, offset[4], offroad_min, offroad_max, max_route_percentage, speed_threshold, max_time, completion_tol;
} adx_drive_cfg;
size_t adx_drive_state_bytes(int32_t scenes);
int adx_drive_reset(void* state, int32_t scenes, const uint8_t* mask /* or NULL: all */, int32_t* done /* or NULL */, adx_stream s);
int adx_drive_step(const adx_drive_cfg* c, const double* pose, const float* velocity, const float* yaw_rate, const double* route,
                   const int32_t* len, const double* cum, const double* discs /* or NULL */, const double* boxes /* or NULL */,
                   void* state, int32_t* done, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Signals v1: the traffic lights and stop signs of a closed loop, advanced by one tick for every scene in one launch -- which stop
 * lines bind the ego right now, as the half-planes cost guidance v1 takes, and the two criteria the reference applies to every
 * drive besides collisions, route deviation and blocked: RunRedLight and RunStopSign (carla_gym/core/task_actor/common/criteria/
 * run_red_light.py, run_stop_sign.py).  One wave per scene, no host decision, capturable; the records live in device memory.
 * Callers and fixtures depend on this definition -- a change is a new version, never an edit.
 *
 *   inputs   signals fp64 [scenes][N][10] in world metres and seconds, 1 <= N <= 64, slot j =
 *              (ax, ay, bx, by, kind, reach, offset, green, yellow, red):
 *            the stop line is the segment A B; kind 1.0 is a light, 2.0 a stop sign, anything else an EMPTY slot.  A slot is
 *            also empty when L = |B - A| is not > 0 or reach is not > 0, and a light when one of green, yellow, red is negative or
 *            NaN or cycle = (green + yellow) + red is not > 0.  |v| = sqrt(v.x * v.x + v.y * v.y).
 *            pose fp64 [scenes][3] as ego frame v1 takes it (a NaN compass counts as 0), p = (pose.x, pose.y); velocity fp32
 *            [scenes], widened exactly; hold int32 [scenes] or NULL.
 *   state    adx_signals_state_bytes(scenes) = 64 * scenes bytes; per scene twelve int32
 *              ticks, have, target (slot + 1; 0 = none), stop_done, red_runs, stop_runs, stops_met, first_tick, first_slot,
 *              emitted (by this step), flags, 0
 *            then two fp64 qx, qy: the probe of the previous step.  All zero bytes = fresh.  A scene's state is read completely
 *            before any word of it is written.  Everything below is fp64 without contraction, every product and sum rounded on
 *            its own, in this order; a NaN makes every comparison it enters false.
 *   slot j   d = B - A;  t = (d.x / L, d.y / L);  n = (-t.y, t.x).  The caller orders A and B so that n points the way the
 *            governed traffic drives: with A = c - w/2 (sin yaw, -cos yaw) and B = c + w/2 (sin yaw, -cos yaw), n is the heading
 *            (cos yaw, sin yaw).  r = p - A;  lon = n.x * r.x + n.y * r.y;  lat = t.x * r.x + t.y * r.y.
 *            forward = (-c, -s) of ego frame v1's (c, s) = (cos, sin)(compass + pi/2), the same two library calls;
 *            head = n.x * forward.x + n.y * forward.y.
 *              gate   = live && lon <= 0 && lon >= -reach && lat >= 0 && lat <= L && head > min_cos
 *              beyond = live && lon > 0 && lat >= 0 && lat <= L
 *   clock    a scene's first step (have == 0) is at time 0: ticks = 0.  Every later step first does ticks += 1.
 *            tm = (double)ticks * dt.  A light: tau = fmod(tm + offset, cycle), + cycle when tau < 0; phase GREEN (1) when
 *            tau < green, YELLOW (2) when tau < green + yellow, else RED (3).  A stop sign's phase is 4, an empty slot's 0.
 *   red run  the reference's tail-segment test, swept over the tick.  q = p + probe * forward (q.x = p.x + probe * forward.x);
 *            q_prev = (qx, qy) of the state; skipped on a scene's first step.  s = q_prev - A, v = q - A;
 *            l0 = n.x * s.x + n.y * s.y;  l1 = n.x * v.x + n.y * v.y.  A crossing needs l0 <= 0 && l1 > 0; then u = l0 / (l0 - l1),
 *            m0 = t.x * s.x + t.y * s.y, m1 = t.x * v.x + t.y * v.y, mc = m0 + u * (m1 - m0), hit = mc >= 0 && mc <= L.
 *            hit && phase == RED adds one to red_runs, the slots taken in index order.
 *   stops    one machine per scene, after the lights, on the state's target as the step found it:
 *              target == 0: the lowest-index slot that is a stop sign and gated, if any, becomes the target; then stop_done = 0
 *                           and stops_met += 1.
 *              target != 0: velocity < speed_threshold sets stop_done = 1.  Then, when the target is not gated (any more):
 *                           stop_runs += 1 when beyond[target] && !stop_done; the target is cleared.
 *            So a target is taken at one step and judged from the next one on, and a sign is not taken at the step that clears
 *            another.
 *   first    the first infraction of a drive (red_runs == 0 && stop_runs == 0 in the state the step found) stores first_tick =
 *            the new `ticks` and first_slot = its slot, a light's (the lowest) before the sign's.  An infraction needs an earlier
 *            step, so first_tick == 0 says "none yet".
 *   emit     after the machine.  A gated light emits when RED, or YELLOW with stop_on_yellow != 0.  A gated stop sign emits
 *            unless it is the (new) target and stop_done is set.  The emitting slots, in index order, fill the first slots of
 *            planes fp32 [scenes][P][3]: ego frame v1's kind 2 of the world plane (n.x, n.y, (n.x * ax + n.y * ay) - margin) --
 *            "stay `margin` metres behind the line".  Every remaining slot is the inert plane (0, 0, 1).  When more than P slots
 *            emit the lowest P are kept and bit 0 of `flags` is set for good.  emitted = the planes written, at most P.
 *   outputs  planes; phase int32 [scenes][N]; the state with have = 1 and (qx, qy) = q.
 *   hold     where hold != 0 the record is FROZEN (the clock included), every plane is inert and phase is still written, for the
 *            time the step would have had.
 *   launch   one workgroup of one wave per scene, lane j owns slot j.  A ballot of the emitting lanes and the population count of
 *            the bits below a lane give its plane slot; the lowest set bit of the gated-stop ballot is the new target.  Lane 0
 *            forms the record, lanes 0 .. 15 store one 32-bit word of it each.  No atomics.
 *   differs  from the reference's two criteria, on purpose.  RunRedLight intersects a short tail segment of the ego (from 0.8 to
 *            1.0 + 1 m of its half-length behind the centre) with the stop line of a red light of the tail's lane, at the tick's
 *            pose, and does not count the same light twice in a row; here ONE tail point, `probe` along the heading, is swept from
 *            its previous to its present place, so a line is not missed between two ticks, every crossing on red counts, and a
 *            line is whatever segment the caller lays down -- nothing reads a map, and neither the lane nor the heading is
 *            asked at a crossing (n orders the sides).  RunStopSign finds its sign through CARLA's trigger volume
 *            and a lane look-ahead, judges the stop while the ego's location is inside the volume, and counts an infraction when
 *            the ego is no longer affected; here the gate box (reach behind the line, the line's width, the heading test) stands
 *            in for volume and look-ahead, and ONLY LEAVING ACROSS THE LINE counts as a run: a target left sideways or backwards
 *            is cleared without one.  Neither criterion ends a drive; the leaderboard's factors (0.7 per light, 0.8 per sign,
 *            leaderboard/utils/statistics_manager.py) are the caller's arithmetic.
 *   rounding the planes differ between two evaluations as ego frame v1's kind 2 says (the b column involves no cos or sin and is
 *            the same number); qx, qy by |probe| * 8 * 2^-52 plus an ulp of the coordinate; every integer of the record is the
 *            same as long as head - min_cos and, with probe != 0, l0, l1, mc and mc - L stay clear of 0 (tests/signals_ref.py).
 *
 * adx_signals_reset zeroes the records of every scene (mask NULL) or of the scenes whose mask byte is not 0, and makes their
 * n_planes planes inert when planes_out is given: one small capturable launch.  adx_signals_state_bytes is 0 for a value out of
 * range.
 *
 * Limits: 1 <= scenes <= 65535, 1 <= n_signals = N <= 64, 1 <= n_planes = P <= 8; dt and xy_scale finite and > 0; margin and
 * speed_threshold finite and >= 0; probe finite (the reference's tail point is -2); -1 <= min_cos < 1.  ADX_ERR_INVALID before
 * any GPU work, each with its own text, for a value out of range, a NULL pointer, or an output (the state, planes, phase) that
 * overlaps an input or another output.
 * -----------------------------------------------------------------------------------*/
typedef struct adx_signals_cfg {
  int32_t scenes, n_signals, n_planes, stop_on_yellow;
  double dt, xy_scale, margin, probe, min_cos, speed_threshold;
} adx_signals_cfg;
size_t adx_signals_state_bytes(int32_t scenes);
int adx_signals_reset(void* state, int32_t scenes, const uint8_t* mask /* or NULL: all */, float* planes_out /* or NULL */,
                      int32_t n_planes, adx_stream s);
int adx_signals_step(const adx_signals_cfg* c, const double* signals, const double* pose, const float* velocity,
                     const int32_t* hold /* or NULL */, void* state, float* planes, int32_t* phase, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Traffic v1: the other road users of a closed loop as car-following agents on caller-laid paths, advanced by one tick for every
 * scene in one launch -- each follows the Intelligent Driver Model behind the nearest of another agent on its path, the ego, and a
 * stop line of signals v1 that shows red or yellow -- and written out as the boxes ego frame v1 and drive metrics v1 take.  What
 * the reference gets from CARLA: its zombie vehicles are on autopilot and its scenario actors run BasicAgent (carla_gym/core/
 * task_actor/scenario_actor/agents/basic_agent.py: a route plan, full brake on a vehicle hazard ahead, a red light or the
 * destination), of which this law's brake-or-go limit is the degenerate case.  One wave per scene, no host decision, capturable;
 * the state lives in device memory.  Callers and fixtures depend on this definition -- a change is a new version, never an edit.
 *
 * NO LIBRARY CALL lies on the way to any state or output word: only IEEE + - * / and sqrt, fp64 without contraction, every
 * product and sum rounded on its own, in the order written here; a NaN makes every comparison it enters false.  So two
 * evaluations of the contract agree in every bit.  Headings therefore come in as a table, and the ego's speed along a path is a
 * progress rate, not a cosine.
 *
 *   inputs   all in device memory, world metres and seconds.
 *            paths fp64 [scenes][Q][G][2], plen int32 [scenes][Q] (clamped into 0..G by the kernel; below 2 the path is EMPTY),
 *            cum fp64 [scenes][Q][G] as drive metrics v1 defines it per path (cum[0] = 0, a sequential sum by the caller;
 *            `length` of a path = cum[plen-1]), heading fp64 [scenes][Q][G]: heading[g] is the world angle of segment g -> g+1,
 *            computed by the caller and only ever copied into a box's yaw.  1 <= Q <= 8, 2 <= G <= 64.
 *            agents fp64 [scenes][N][9], 1 <= N <= 64, slot i =
 *              (path, start_s, start_v, desired_v, length, width, headway, accel, brake).
 *            A slot is EMPTY when path is not an integer in 0..Q-1 or names an empty path; when length, width, desired_v, accel
 *            or brake is not > 0; when headway, start_s or start_v is negative or NaN; when start_s is not below its path's length.
 *            stops fp64 [scenes][T][3] = (path, s_stop, signal slot), 0 <= T <= 16, and phase int32 [scenes][n_signals], the
 *            output of signals v1 (2 yellow, 3 red) read as it stands at the launch: both NULL exactly when T = 0.  A stop is
 *            INERT when its path is not the agent's, when its slot is not an integer in 0..n_signals-1, or when its phase is
 *            neither 2 nor 3.
 *            pose fp64 [scenes][3], pos = (pose.x, pose.y), the compass is not read; velocity fp32 [scenes] is carried for the
 *            record only (v1 does not read it; a later version may); hold int32 [scenes] or NULL.
 *   state    adx_traffic_state_bytes(scenes, N) = 4 * W * scenes bytes, W = 32 + 5 N + (N odd ? 1 : 0) 32-bit words per scene:
 *              word 0 ticks, 1 have, 2 arrived, 3 ego_yields, 4 ego_hard, 5 overlaps (int32), 6..7 min_ego_gap (fp64),
 *              8..23 se_prev[8] (fp64: the ego's arc length on path q at the previous step), 24..31 on_prev[8] (int32: whether it
 *              was on path q then), 32.. s[N] (fp64), then v[N] (fp64), then alive[N] (int32), then a zero word when N is odd.
 *            All zero bytes = fresh: a step that finds have == 0 first takes the state adx_traffic_reset leaves (below).  A
 *            scene's state is read completely before any word of it is written.  Agent i is LIVE when alive[i] != 0 and its slot
 *            is not empty at this launch.  Every agent sees the OLD s, v of every other agent (a synchronous update).
 *   ego      for every path q that is not empty the position is projected as drive metrics v1's `progress` does it, over ALL
 *            segments j in 0..plen-2 (no cursor, no window): a = p[j], u = p[j+1] - a, L2 = u.x * u.x + u.y * u.y;  t = 0 when
 *            not L2 > 0, else ((pos.x - a.x) * u.x + (pos.y - a.y) * u.y) / L2 clamped into 0..1 (a NaN becomes 0);  c = (a.x +
 *            t * u.x, a.y + t * u.y);  d = sqrt((pos.x - c.x)^2 + (pos.y - c.y)^2), a NaN d counting as +inf.  The smallest d
 *            wins, the LOWER j on a tie.  se = cum[j] + t * sqrt(L2);  on_q = d <= lane_half_width.  When on_q holds and held at
 *            the previous step too (on_prev[q], and have != 0): ue = max((se - se_prev[q]) / dt, 0), a NaN becoming 0; otherwise
 *            ue = 0: a road user that has just appeared, or is crossing, counts as standing.  The new se_prev[q] = se and
 *            on_prev[q] = on_q; an empty path's are 0.
 *   leader   of live agent i on path p, with front = s_i + length_i / 2.  The candidates, each a rear position r and a speed u:
 *              1. every other live agent k on path p, k = 0, 1, ..., with s_k > s_i, or s_k == s_i && k < i:
 *                 r = s_k - length_k / 2, u = v_k;
 *              2. the ego when on_p and se > s_i: r = se - ego_length / 2, u = ue;
 *              3. every stop t = 0, 1, ... that is not inert and BINDS: front <= s_stop and its phase is RED, or front <= s_stop,
 *                 its phase is YELLOW and (s_stop - front) * (2 * brake_i) >= v_i * v_i (it can still stop comfortably; otherwise
 *                 it goes through): r = s_stop, u = 0.
 *            The smallest r wins; a tie goes to the earlier candidate in this order.  leader int32 [scenes][N] is an output:
 *            -1 none (or not live), 0..63 an agent, 64 the ego, 65 + t stop t.
 *   law      f = v / desired_v;  free = 1 - (f * f) * (f * f).  With a leader: gap = r - front;
 *            star = jam + max(0, v * headway + (v * (v - u)) / (2 * sqrt(accel * brake))) (a NaN inside max becoming 0);
 *            g = max(gap, gap_min) (a NaN becoming gap_min);  inter = (star / g) * (star / g).  Without one inter = 0.
 *            acc = accel * (free - inter);  acc < -brake_max sets acc = -brake_max and marks the tick HARD;  acc > accel sets
 *            acc = accel.  v' = max(0, v + acc * dt) (a NaN becoming 0);  s' = s + v' * dt: semi-implicit, as vehicle v1.
 *   record   ticks += 1;  ego_yields += the live agents whose leader is the ego;  ego_hard += those of them whose tick is hard
 *            (the ego cut someone off);  overlaps += the live agents with an agent leader and gap < 0 (0 in every sane run);
 *            min_ego_gap = min(min_ego_gap, the gaps of the agents the ego leads), +inf until it leads someone.
 *   arrival  s' >= its path's length retires the agent: alive = 0 and arrived += 1.  A live agent stores s', v'; every other
 *            slot stores its s, v again.
 *   boxes    fp64 [scenes][N][7] = (cx, cy, vx, vy, yaw, length, width), drive metrics v1's format.  For an agent that is live
 *            after the step: j = the largest index in 0..plen-2 with cum[j] <= s' (0 when there is none);  e = p[j+1] - p[j],
 *            L = sqrt(e.x * e.x + e.y * e.y), unit = (e.x / L, e.y / L), or 0 when not L > 0;  centre = (p[j].x + (s' - cum[j]) *
 *            unit.x, ...);  velocity = (v' * unit.x, v' * unit.y);  yaw = heading[j];  length and width as given.  An empty,
 *            dead or retired slot is seven zeros (length 0 = empty everywhere downstream).
 *   reset    adx_traffic_reset puts the agents of every scene (mask NULL) or of the scenes whose mask byte is not 0 at start_s,
 *            start_v with alive = 1 (an empty slot: 0, 0, 0), zeroes the record and the ego's path memory, sets have = 1 and
 *            min_ego_gap = +inf, WRITES THEIR BOXES, and their leader = -1 when `leader` is given: the boxes are valid before the
 *            first step, no priming step is needed.  One small capturable launch.
 *   hold     where hold != 0 the scene is FROZEN: no word of its state or of leader is written and its boxes are written again
 *            from the state as it stands.
 *   launch   one workgroup of one wave per scene, lane i owns agent i.  The scene's paths are staged into LDS once (at most 16
 *            KB).  The ego is projected path by path, lanes over segments, with drive metrics v1's xor butterfly over (d, j).
 *            The leader search is a uniform loop over k with a broadcast of lane k's (path, s, v, rear); the stops are a short
 *            uniform loop.  The counters are population counts of ballots.  Lane 0 forms the record, lanes 0 .. 31 store one
 *            32-bit word of it each; every lane stores its agent and its box one 32-bit word per instruction.  No atomics.
 *   differs  from BasicAgent, on purpose.  It brakes fully when a vehicle is inside 9.5 m and a 45 degree cone ahead and
 *            otherwise follows its plan with a PID; here a continuous law (IDM) gives the approach, the queue and the start-up,
 *            and "ahead" is membership of the same path, not a cone -- nothing here reads a map.  There are no walkers and no
 *            lane changes.  There is no junction priority: paths that cross do not see each other.  The ego is seen where it is
 *            within lane_half_width of a path, at the speed it has made along that path since the previous step.  Agents do NOT
 *            obey stop signs: a stop whose phase is 4 is inert.
 *   rounding every word of the state, of boxes and of leader is the same in two evaluations: there is no library call to differ in.
 *
 * adx_traffic_state_bytes is 0 for a value out of range.
 *
 * Limits: 1 <= scenes <= 65535, 1 <= n_agents = N <= 64, 1 <= n_paths = Q <= 8, 2 <= n_points = G <= 64, 0 <= n_stops = T <= 16,
 * n_signals <= 64 and >= 1 when T > 0 (>= 0 otherwise); dt, lane_half_width, ego_length, jam, gap_min (the floor under a gap before
 * it is divided by) and brake_max (the hard cap on deceleration) finite and > 0.  ADX_ERR_INVALID before any GPU work, each with
 * its own text, for a value out of range, a NULL pointer (stops and phase not NULL exactly when T > 0; hold, the mask and reset's
 * leader may be NULL), or an output (the state, boxes, leader) that overlaps an input or another output.
 * -----------------------------------------------------------------------------------*/
typedef struct adx_traffic_cfg {
  int32_t scenes, n_agents, n_paths, n_points, n_stops, n_signals;
  double dt, lane_half_width, ego_length, jam, gap_min, brake_max;
} adx_traffic_cfg;
size_t adx_traffic_state_bytes(int32_t scenes, int32_t n_agents);
int adx_traffic_reset(const adx_traffic_cfg* c, const double* paths, const int32_t* plen, const double* cum, const double* heading,
                      const double* agents, const uint8_t* mask /* or NULL: all */, void* state, double* boxes,
                      int32_t* leader /* or NULL */, adx_stream s);
int adx_traffic_step(const adx_traffic_cfg* c, const double* paths, const int32_t* plen, const double* cum, const double* heading,
                     const double* agents, const double* stops /* or NULL */, const int32_t* phase /* or NULL */,
                     const double* pose, const float* velocity, const int32_t* hold /* or NULL */, void* state, double* boxes,
                     int32_t* leader, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Camera v1: the front camera of a closed loop, rendered on the device -- an analytic ray caster over exactly the primitives the
 * loop already holds (the ground with its roads and stop lines, the world's boxes and discs, the lamps and poles of its signals),
 * one C call per tick that writes the frame the encoder reads.  The reference closes its loop through CARLA's RGB sensor
 * (e2e_driving/diffusion_agent.py: sensors(): 900 x 256, fov 100 degrees, 1.5 m behind the vehicle centre, 2.0 m up, pitch 0); this
 * package rules the simulator out, so the renderer is its own.  Capturable: no allocation, no synchronisation, no host decision.
 * Callers and fixtures depend on this definition -- a change is a new version, never an edit.
 *
 *   frame    the camera frame is ego frame v1 in METRES (`rotate` and `point` with xy_scale 1: x lateral, +y forward) plus z up,
 *            moved so that the eye is the origin: a world point (X, Y) at height Z is
 *              (x, y) = rotate(X - px, Y - py);  cam = (x, y - mount_back, Z - cam_height)
 *            -- the eye sits at ego (0, mount_back, cam_height); the reference's mount is mount_back = -1.5, cam_height = 2.0.
 *            The ground is the plane z = -cam_height.  v1 has no pitch and no roll.  Columns increase towards +x, rows downwards.
 *   ray      of pixel (u, v), all fp32: dx = ((u + 0.5) - W/2) * k;  dy = 1;  dz = -(((v + 0.5) - H/2) * k);  k = 2 tan(fov / 2) / W
 *            formed on the host in fp64 and rounded to fp32 once (square pixels).  Rays are not normalised: the parameter t of a
 *            point t * (dx, 1, dz) is its forward depth.  A2 = dx * dx + 1;  A3 = A2 + dz * dz.
 *   stage    the first of the call's two launches, one wave per scene: every primitive into the camera frame in fp64, no
 *            contraction, every product and sum rounded on its own in the order written here, with ego frame v1's (c, s) -- the
 *            same two library calls -- and each word rounded to fp32 ONCE into the table `prims` (the caller's workspace of
 *            adx_camera_prims_bytes(cfg) bytes, 16-byte aligned).  Per scene the table is 16 int32 header words (1, n_obj, n_gnd,
 *            0 ...), n_obj = n_boxes + n_discs + 2 n_signals OBJECT records of 16 words in the order boxes, discs, lamps, poles,
 *            and n_gnd = n_signals + n_paths * (n_points - 1) GROUND records of 8 words in the order stop lines, road segments
 *            (path-major).  An object record: word 0 int32 key = class << 8 | slot, 0 = EMPTY (the whole record is then zero);
 *            words 1..4 int32 (u0, u1, v0, v1), a pixel rectangle, inclusive, outside which no ray hits the object (below);
 *            words 5.. by class; the rest zero.  A ground record: (ax, ay, ex, ey, inv, live int32, 0, 0), EMPTY = all zero.
 *   box j    class 5 over boxes[s][j] = (cx, cy, vx, vy, yaw, length, width), drive metrics v1's format; hl = length / 2, hw =
 *            width / 2;  b = point(cx, cy);  a = rotate(cos yaw, sin yaw): the length axis; the width axis is (-a.y, a.x); z from
 *            zlo = -cam_height to zhi = zlo + box_height.  The eye in the box's axes: el = -(b.x * a.x + b.y * a.y),
 *            ew = b.x * a.y - b.y * a.x.  Words 5..12 = (a.x, a.y, -hl - el, hl - el, -hw - ew, hw - ew, zlo, zhi).  EMPTY when hl
 *            or hw is not > 0, or the eye is inside (|el| <= hl, |ew| <= hw, zlo <= 0 <= zhi).
 *            Pixel: dl = dx * a.x + a.y;  dw = a.x - dx * a.y;  the slab test over the axes 0 (length: dl, words 7, 8), 1 (width:
 *            dw, words 9, 10), 2 (z: dz, words 11, 12) in this order, from tn = -inf, tf = +inf: d == 0 is handled explicitly -- a
 *            miss unless n0 <= 0 <= n1, never a division; otherwise t1 = n0 / d, t2 = n1 / d, (lo, hi) = (t1, t2) when d > 0, else
 *            (t2, t1); lo > tn sets tn = lo and the ENTERED FACE = 0 (-length), 1 (+length), 2 (-width), 3 (+width), 4 (top): 2 *
 *            axis + (d > 0 ? 0 : 1), always 4 for z (strictly greater: on a tie the lower axis wins); hi < tf sets tf = hi.  A hit
 *            when tn <= tf, at t = tn.  The id is face << 16 | 5 << 8 | j.
 *   disc j   class 6 over discs[s][j] = (cx, cy, vx, vy, r): a vertical cylinder, c = point(cx, cy), zlo = -cam_height, zhi = zlo +
 *            disc_height, r2 = r * r.  Words 5..9 = (c.x, c.y, r2, zlo, zhi).  EMPTY when r is not > 0 or the eye is inside
 *            ((c.x * c.x + c.y * c.y) - r2 <= 0 and zlo <= 0 <= zhi).
 *            Pixel: B = dx * c.x + c.y;  cr = dx * c.y - c.x (direction x centre: no cancellation between large terms, unlike
 *            B * B - A2 * |c|^2);  disc = A2 * r2 - cr * cr.  SIDE when disc >= 0: ts = (B - sqrt(disc)) / A2, a hit when
 *            zlo <= ts * dz <= zhi.  CAP when dz < 0: tc = zhi / dz, x = dx * tc - c.x, y = tc - c.y, a hit when x * x + y * y <= r2.
 *            Both are candidates of the hit rule with the same id 6 << 8 | j.
 *   lamp j   class 7, for signals[s][j] (signals v1's record) with phase[s][j] in 1..4 and L = |B - A| > 0; any other slot leaves
 *            its lamp, pole and stop line EMPTY.  With signals v1's t = (B - A) / L and n = (-t.y, t.x) (the driving direction):
 *            m = A + 0.5 * (B - A);  w = m + lamp_setback * n (a far-side signal);  l = (point(w), lamp_height - cam_height);
 *            R2 = lamp_radius^2.  Words 5..9 = (l.x, l.y, l.z, R2, phase int32).  EMPTY when ((l.x * l.x + l.y * l.y) + l.z * l.z) -
 *            R2 is not > 0 (the eye inside).  Pixel: B = (dx * l.x + l.y) + dz * l.z;  c = (l.y * dz - l.z, l.z * dx - l.x * dz,
 *            l.x - l.y * dx);  disc = A3 * R2 - ((c.x * c.x + c.y * c.y) + c.z * c.z);  a hit when disc >= 0 at
 *            t = (B - sqrt(disc)) / A3.
 *   pole j   class 8: disc j's arithmetic for the cylinder of pole_radius over point(w) from the ground to the lamp's centre, zhi
 *            = l.z (pole_radius 0: none).
 *   line j   the stop line of a signal that is not empty, ground record j: a = point(A), e = point(B) - a, inv = 1 / (e.x * e.x +
 *            e.y * e.y), or 0 when that is not > 0; live = 1.
 *   road     roads fp64 [scenes][Q][G][2] and road_len int32 [scenes][Q] -- traffic v1's `paths` and `plen` as they are; a length
 *            is clamped into 0..G and a path with fewer than 2 counted points has no segment.  Segment g of path q (g + 1 <
 *            len), ground record n_signals + q (G - 1) + g: a stop line's arithmetic on the points g and g + 1; live = 0 when a
 *            coordinate is NaN.
 *   ground   a ray with dz < 0 meets the ground at tg = cam_height / (-dz), at (gx, gy) = (dx * tg, tg).  Squared distance to a
 *            ground record by clamped projection: q = g - a;  u = (q.x * e.x + q.y * e.y) * inv;  u < 0 becomes 0, u > 1 becomes 1;
 *            c = (q.x - u * e.x, q.y - u * e.y);  d2 = c.x * c.x + c.y * c.y.  The ground's id, in this order:
 *              tg > far                                 1 << 8 | 1   far ground
 *              d2 <= line_half^2 for a live stop line   4 << 8 | j   the lowest such j; wins over road and marking
 *              dmin = the smallest d2 over the live road segments (+inf without one):
 *              dmin < (half_width - mark)^2             2 << 8       road
 *              dmin <= half_width^2                     3 << 8       edge marking
 *              otherwise                                1 << 8       ground
 *            The three squared thresholds are formed on the host in fp64 and rounded to fp32 once.
 *   hit      a candidate counts when t > near.  The nearest t wins; on an exact tie the lower class << 8 | slot wins, the ground
 *            (class 1 for this purpose) before every object.  Nothing hit: sky, id 0, depth +inf.  A primitive the eye is inside
 *            is empty (stage).  A NaN makes every comparison it enters false.
 *   pixel    fp32 only: + - * / sqrt and comparisons, each rounded on its own (no contraction, no fast-math, no library call), so
 *            a float32 restatement run on the same table makes the same decisions (tests/camera_ref.py).
 *   cull     words 1..4 of an object record come from the eight corners of its bounding cuboid in fp64, each projected and
 *            widened outwards by one pixel plus 2^-20 of the corner's coordinates carried through the projection.  A corner
 *            nearer than 0.05 m to the eye's plane, or a NaN, makes the rectangle the whole image (-1, 2^20, -1, 2^20); every
 *            corner behind that plane makes it empty (1, 0, 1, 0).  A culled evaluation gives the plain loop's answer.
 *   colour   flat, from palette uint8 [20][3]: 0 sky; 1 ground; 2 far ground; 3 road; 4 marking; 5 stop line; 6 + (j % 8) box j;
 *            14 disc; 15 pole; 16 + (phase - 1) lamp.  A box face is shaded in integers, (c * shade[face]) >> 8.  A pixel's colour
 *            is a pure function of its id and its signal's phase.  adx_camera_default_palette writes the committed default.
 *   outputs  each optional, at least one: frames uint8 [scenes][H][W][3] (adx_resnet_forward_frames' format); image fp32
 *            [scenes][3][H][W]: bit for bit what adx_image_normalize makes of `frames` with cfg's mean and std, ((float)c / 255 -
 *            mean) / std; ids int32 [scenes][H][W]; depth fp32 [scenes][H][W]: t, +inf for sky.
 *   hold     int32 [scenes] or NULL: where hold != 0 neither the scene's table nor any of its outputs is written.
 *   launch   stage: one workgroup of one wave per scene, lane j owns box, disc and signal j, the lanes stride over the segments.
 *            render: one workgroup of 256 threads per 64 x 16 tile of a scene; the objects whose rectangle meets the tile are
 *            compacted into LDS by ballot in index order, the ground records are copied by tiles that reach below the horizon;
 *            one lane per pixel, every lane of a wave on the same record.  A full, word-aligned row of frames goes out as packed
 *            32-bit words.  No atomics.
 *   differs  from the reference's sensor, on purpose and by far: flat-shaded geometry, not a town.  No textures, no lighting, no
 *            fog, no shadows, no anti-aliasing, no lens model, no continuous term of any kind; the road is a distance to
 *            polylines; other road users are cuboids, signals a sphere on a pole.  CARLA-trained weights do not transfer.
 *   rounding two evaluations of `stage` that differ only in their cos and sin routines (each within 4 ulp) differ per position word
 *            as ego frame v1's `point` says -- one fp32 ulp plus 8 * 2^-52 * (|dx| + |dy|) -- and per derived word by that carried
 *            through its products (tests/camera_ref.py derives each); the render launch is exact on a given table.
 *
 * adx_camera_prims_bytes is 0 for a count out of range, else 4 * scenes * (16 + 16 n_obj + 8 n_gnd).
 *
 * Limits: 1 <= scenes <= 65535, 8 <= width <= 2048, 8 <= height <= 1024, 0 < fov < 3 rad, 0 <= n_boxes, n_discs, n_signals <= 64,
 * 0 <= n_paths <= 8 with 2 <= n_points <= 64 (n_points = 0 when n_paths = 0); mount_back and lamp_setback finite; cam_height, near,
 * far > near, half_width, line_half, box_height, disc_height, lamp_radius, lamp_height finite and > 0; 0 <= mark <= half_width;
 * pole_radius finite and >= 0; mean finite, std finite and not 0.  ADX_ERR_INVALID before any GPU work, each with its own text, for
 * a value out of range, a NULL pointer that a count above 0 needs (pose and prims always), prims not 16-byte aligned, no output at
 * all, or an output (prims, frames, image, ids, depth) that overlaps an input or another output.
 * -----------------------------------------------------------------------------------*/
#define ADX_CAMERA_PALETTE 20
typedef struct adx_camera_cfg {
  int32_t scenes, width, height, n_boxes, n_discs, n_signals, n_paths, n_points;
  double fov, mount_back, cam_height, near, far, half_width, mark, line_half, box_height, disc_height, lamp_radius, lamp_height,
      lamp_setback, pole_radius;
  float mean[3], stdv[3];
  uint8_t palette[ADX_CAMERA_PALETTE][3];
  uint8_t shade[5];
  uint8_t reserved[7];
} adx_camera_cfg;
size_t adx_camera_prims_bytes(const adx_camera_cfg* c);
void adx_camera_default_palette(uint8_t* palette /* [20][3] or NULL */, uint8_t* shade /* [5] or NULL */);
int adx_camera_render(const adx_camera_cfg* c, const double* pose, const double* boxes /* or NULL */, const double* discs /* or NULL */,
                      const double* signals /* or NULL */, const int32_t* phase /* or NULL */, const double* roads /* or NULL */,
                      const int32_t* road_len /* or NULL */, const int32_t* hold /* or NULL */, void* prims,
                      uint8_t* frames /* or NULL */, float* image /* or NULL */, int32_t* ids /* or NULL */,
                      float* depth /* or NULL */, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Expert v1: a privileged driver for every scene of a launch -- it sees the world and not the pixels: it follows the route window,
 * queues behind whatever is nearest ahead of it in its corridor (a box, a disc, a stop plane of signals v1, the end of the route)
 * by traffic v1's Intelligent Driver Model, slows for bends, and writes the plan control v1 takes as it is.  What the reference
 * collects its demonstrations with is CARLA's autopilot and a Roach expert (misc/data_collect.py); this package rules the
 * simulator out, so the expert is its own.  A STATELESS launch: one workgroup of one wave per scene, no atomics, no host decision,
 * capturable.  Callers and fixtures depend on this definition -- a change is a new version, never an edit.
 *
 * NO LIBRARY CALL lies on the way to any output word: only IEEE + - * / and sqrt in fp64 without contraction, every product, sum,
 * division and square root rounded on its own, in the order written here; headings arrive as unit vectors, curvature is Menger's,
 * there is no trigonometry.  A NaN makes every comparison it enters false.  So two evaluations agree in every bit.
 *
 *   inputs   all in device memory, in a tick's ego frame (ego frame v1) and model units, fp32, every word widened exactly to fp64.
 *            A length becomes metres by `* xy_scale`; an obstacle velocity w becomes m/s by (w * xy_scale) / waypoint_dt.
 *            window fp32 [scenes][R][2]: route planner v1's window, 2 <= R <= 32, best with first = 0;  P[i] = (x * xy_scale,
 *            y * xy_scale).  velocity fp32 [scenes] m/s;  v_0 = velocity when velocity > 0, else 0 (a NaN becomes 0).
 *            boxes fp32 [scenes][N][8] = adx_world_to_ego's kind 3 (cx, cy, vx, vy, hx, hy, length, width), 0 <= N <= 64, NULL
 *            exactly when N = 0; a slot is EMPTY unless length > 0 and width > 0.  The heading (hx, hy) is used as it stands.
 *            discs fp32 [scenes][M][5] = kind 1 (cx, cy, vx, vy, radius), 0 <= M <= 64, NULL exactly when M = 0; EMPTY unless
 *            radius > 0.  planes fp32 [scenes][K][3] = (nx, ny, b), signals v1's output (n . p <= b is the allowed side),
 *            0 <= K <= 8, NULL exactly when K = 0;  bm = b * xy_scale, n as it stands.
 *   path     segment j = 0 .. R-2:  e_j = P[j+1] - P[j];  L2_j = e.x * e.x + e.y * e.y.  A segment whose L2 is not > 0 is
 *            DEGENERATE: len_j = 0, tau_j = (0, 0), and a projection onto it has t = 0.  Otherwise len_j = sqrt(L2_j) and
 *            tau_j = (e.x / len_j, e.y / len_j).  cum[0] = 0, cum[j+1] = cum[j] + len_j, the sequential sum; total = cum[R-1].
 *            The path ENDS when segment R-2 is degenerate (route planner v1 pads a window with the route's last point).
 *   project  of a point q in metres, traffic v1's rule over all segments: a = P[j];  t = 0 on a degenerate segment, else
 *            f = ((q.x - a.x) * e.x + (q.y - a.y) * e.y) / L2 clamped into 0..1 (a NaN becomes 0);  c = (a.x + t * e.x,
 *            a.y + t * e.y);  d = sqrt((q.x - c.x)^2 + (q.y - c.y)^2), a NaN d counting as +inf.  The smallest d wins, the
 *            LOWER j on a tie.  s = cum[j] + t * len_j.  It gives (s, d, j) and the point c.  The ego is the origin: (s_e,
 *            d_e, j_e) and c_e.  ONE EXCEPTION to the clamp: on segment 0, f < 0 gives t = f -- THE PATH BEGINS WITH A RAY.
 *            Route planner v1 pops every point within min_distance of the ego, so its window begins at the farthest of them,
 *            up to min_distance AHEAD of the ego; clamped there, the ego and everything between it and P[0] would collapse
 *            onto P[0].  On the ray s is negative, and arc lengths are only ever compared and subtracted.
 *   leader   the candidates, each a rear position r -- the metres of free road ahead of the ego's front bumper -- and a speed u,
 *            in this order; the smallest r wins, the earlier candidate on a tie; a NaN r never wins:
 *              box i    not empty; c = (cx, cy) * xy_scale projects to (s, d, j);  hl = (length * xy_scale) / 2,
 *                       hw = (width * xy_scale) / 2;  dt_ = |hx * tau_j.x + hy * tau_j.y|,  cr = |hx * tau_j.y - hy * tau_j.x|;
 *                       lon = hl * dt_ + hw * cr;  lat = hl * cr + hw * dt_.  It counts when d <= corridor_half + lat and
 *                       s - s_e > 0.  r = ((s - s_e) - lon) - ego_front;  with vel = ((vx * xy_scale) / waypoint_dt, ...):
 *                       u = max(0, vel.x * tau_j.x + vel.y * tau_j.y), a NaN becoming 0.
 *              disc i   the same with lon = lat = radius * xy_scale.
 *              plane k  g(p) = (n.x * p.x + n.y * p.y) - bm.  INERT when n.x == 0 and n.y == 0, when the origin is already
 *                       beyond it (-bm > 0), or when the path walked from the ego's projection on never passes from g <= 0 to
 *                       g > 0.  The walk: the piece (c_e at arc s_e) -> P[j_e + 1], then the segments j_e + 1 .. R-2, each
 *                       (P[j] at arc cum[j]) -> (P[j+1] at arc cum[j+1]).  The first piece A -> B with ga = g(A) <= 0 and
 *                       gb = g(B) > 0 gives arc = arc_A + (ga / (ga - gb)) * (arc_B - arc_A), a linear interpolation.
 *                       r = (arc - s_e) - ego_front;  u = 0.
 *              the end  when the path ends:  r = ((total - s_e) - ego_front) - end_margin;  u = 0.
 *            leader int32 [scenes] is an output: -1 none, 0..63 box i, 64..127 disc i - 64, 128 + k plane k, 136 the end.
 *   curve    look = look_min + v_0 * look_time.  Over the interior vertices i = 1 .. R-2 whose segments i-1 and i are both not
 *            degenerate and whose ah = cum[i] - s_e satisfies ah >= 0 and ah <= look:  ch = P[i+1] - P[i-1];
 *            lc = sqrt(ch.x * ch.x + ch.y * ch.y);  x = |e_{i-1}.x * e_i.y - e_{i-1}.y * e_i.x|;
 *            kappa = (2 * x) / ((len_{i-1} * len_i) * lc)  (Menger);  where kappa > 0: lim = sqrt(lat_accel / kappa).
 *            desired = min(desired_v, the smallest lim).  Evaluated ONCE per launch, not per roll-out step.
 *   law      traffic v1's, formula for formula, rolled out over k = 0 .. H-1 from v_0 and a_0 = 0 with the leader moving at
 *            constant u:  f = v_k / desired;  free = 1 - (f * f) * (f * f).  With a leader:
 *            gap = (r + u * ((double)k * waypoint_dt)) - a_k;  star = jam + max(0, v_k * headway + (v_k * (v_k - u)) /
 *            (2 * sqrt(accel * brake))) (a NaN inside max becoming 0);  g = max(gap, gap_min) (a NaN becoming gap_min);
 *            inter = (star / g) * (star / g).  Without one inter = 0.  acc_k = accel * (free - inter), set to -brake_max when
 *            below it and to accel when above it.  v_{k+1} = max(0, v_k + acc_k * waypoint_dt) (a NaN becoming 0);
 *            a_{k+1} = a_k + v_{k+1} * waypoint_dt: semi-implicit, as vehicle v1.
 *   rows     row k is the path's point at arc A = s_e + a_k:  j = the largest index of a segment that is not degenerate and has
 *            cum[j] <= A, or the lowest one that is not degenerate when there is none;  p = (P[j].x + (A - cum[j]) * tau_j.x,
 *            ...).  Nothing clamps A to the segment, so beyond the last point the plan continues along the last tangent
 *            (and before the first along the ray).  A path without any such segment gives p = P[0].  Row 0 is the ego's projection onto the path: that is what pulls
 *            the controller back onto the route.
 *   outputs  plan fp32 [scenes][H][D], 2 <= H <= 64, 2 <= D <= 16: columns 0 and 1 = (p.x / xy_scale, p.y / xy_scale), every
 *            other column 0.  leader.  info fp32 [scenes][8] = (s_e, d_e, desired, r, u, acc_0, v_H, a_H), r = +inf and u = 0
 *            without a leader.  Each word is rounded to fp32 once; a NaN is stored as 0x7fc00000.
 *   launch   one workgroup of one wave per scene.  The window is staged into LDS once (points, then the segments, lane j segment
 *            j, then cum by lane 0).  Lane i owns box i, disc i, plane i and curve vertex i, each with a uniform loop over the
 *            segments; an xor butterfly takes the minimum over (r, leader code) and another over lim.  Every lane runs the
 *            H-step roll-out redundantly and keeps a_k when k is its own index; lane k stores row k.  Vector stores only.
 *   differs  from the reference's collectors, on purpose.  CROSSING TRAFFIC IS NOT PREDICTED: an obstacle counts only while it
 *            is inside the corridor, at its speed along the path.  There are NO LANE CHANGES and NO OVERTAKING: a leader that
 *            stands is queued behind for good.  THE CURVE LIMIT IS EVALUATED ONCE PER LAUNCH, at the launch's speed, and holds
 *            for the whole roll-out.  Stop signs bind only as long as signals v1 emits their plane.  Nothing reads a map.
 *   rounding every word of plan, leader and info is the same in two evaluations: there is no library call to differ in.
 *
 * Limits: 1 <= scenes <= 65535, 2 <= window = R <= 32, 0 <= n_boxes, n_discs <= 64, 0 <= n_planes <= 8, 2 <= horizon = H <= 64,
 * 2 <= dim = D <= 16; xy_scale, waypoint_dt, desired_v, accel, brake, brake_max, headway, jam, gap_min, corridor_half, lat_accel
 * and look_time finite and > 0; ego_front, end_margin and look_min finite and >= 0.  ADX_ERR_INVALID before any GPU work, each with
 * its own text, for a value out of range, a NULL pointer that may not be NULL (boxes, discs, planes exactly when their count is
 * 0), or an output (plan, leader, info) that overlaps an input or another output.
 * -----------------------------------------------------------------------------------*/
typedef struct adx_expert_cfg {
  int32_t scenes, window, n_boxes, n_discs, n_planes, horizon, dim, reserved;
  double xy_scale, waypoint_dt, desired_v, accel, brake, brake_max, headway, jam, gap_min, corridor_half, lat_accel, look_time,
      ego_front, end_margin, look_min;
} adx_expert_cfg;
int adx_expert_plan(const adx_expert_cfg* c, const float* window, const float* velocity, const float* boxes /* or NULL */,
                    const float* discs /* or NULL */, const float* planes /* or NULL */, float* plan, int32_t* leader, float* info,
                    adx_stream s);

/* ------------------------------------------------------------------------------------
 * Capsules from boxes v1: the capsule slots of cost guidance v5 from ORIENTED BOXES, one launch -- what a perception stack hands a
 * planner for the other road users.  Capturable: no allocation, no synchronisation, no host decision, so a captured tick whose
 * boxes change at every replay needs no host work.  Callers and fixtures depend on this definition -- a change is a new version,
 * never an edit.
 *
 *   boxes    float32 [scenes][N][8] = (cx, cy, vx, vy, ux, uy, length, width) in device memory, 1 <= N <= 32: centre, velocity per
 *            waypoint, UNIT heading (ux, uy) along `length`, and the two sizes, in cost guidance v5's units and frame.  The
 *            caller normalises the heading, so the device needs no sin or cos and the result can be checked bit for bit; a
 *            heading that is not unit scales the axis, nothing checks it.
 *   inflate  a host scalar by value, finite and >= 0: added to every live capsule's radius -- the ego's own radius.
 *   out      float32 [scenes][N][7]: the slots of adx_guide_capsules, box j of scene s at slot j of scene s.
 *   per box  fp32, no contraction, every operation rounded on its own:
 *              live = length > 0 && width > 0        (a NaN is not live: the slot becomes seven zeros, an empty capsule)
 *              lon  = length >= width
 *              a = lon ? length : width;   b = lon ? width : length
 *              s = a / 2 - b / 2
 *              dx = lon ? ux : -uy;   dy = lon ? uy : ux
 *              ox = s * dx;  oy = s * dy
 *              out = (cx - ox, cy - oy, cx + ox, cy + oy, vx, vy, b / 2 + inflate)
 *            The capsule is the box's INSCRIBED stadium: its axis runs along the longer side (turned by a quarter when the
 *            width is the longer one), and a square box is a disc (s = 0, a == b).  The box's corners stick out of it by up to
 *            (sqrt(2) - 1) * b / 2; `inflate` is where the caller covers that.
 *   launch   one thread per box, 256 threads per workgroup.
 *
 * ADX_ERR_INVALID before any GPU work: NULL boxes or out; n_boxes outside 1..32; scenes < 1 (or above 2^20); an inflate that is
 * negative or not finite; out overlapping boxes.
 * -----------------------------------------------------------------------------------*/
int adx_capsules_from_boxes(const float* boxes, float* out, int32_t scenes, int32_t n_boxes, float inflate, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Cost field from occupancy v1: a cost raster for cost guidance v2 from a binary occupancy raster, one launch.  The value at a
 * node is the disc potential of cost guidance v1 around the NEAREST occupied node: 0.5 on an obstacle, falling to 0 at distance
 * `margin`.  No square root.  Capturable: no allocation, no synchronisation, no host decision.  Callers and fixtures depend on
 * this definition -- a change is a new version, never an edit.
 *
 *   occ      float32 [scenes][gy][gx], 2 <= gx, gy <= 256, 1 <= scenes <= 65535.  A node is occupied iff occ > 0.5f (a NaN is
 *            free).
 *   d2       per node (i, j): the minimum over the occupied nodes (i + di, j + dj) of the raster with |di| <= ry, |dj| <= rx
 *            (0 <= rx, ry <= 16) of  ((float)dj * dx) * ((float)dj * dx) + ((float)di * dy) * ((float)di * dy),  fp32, each
 *            product and the sum rounded on its own.  A minimum is exact: the search order is free.
 *   cells    phi = 1 - d2 * inv_m2;  cells[i][j] = phi > 0 ? (phi * phi) / 2 : 0;  no occupied node in the window: 0.
 *            inv_m2 = fp32(1 / margin^2), formed on the host.  Nodes further than the window see nothing: a caller picks
 *            rx >= margin / dx and ry >= margin / dy.
 *
 * ADX_ERR_INVALID before any GPU work: a NULL pointer; scenes, gx or gy out of range; rx or ry outside 0..16; dx, dy or inv_m2
 * not finite or not > 0; cells overlapping occ.
 * -----------------------------------------------------------------------------------*/
#define ADX_FIELD_MAX_RADIUS 16
int adx_cost_field_from_occupancy(const float* occ, float* cells, int32_t scenes, int32_t gy, int32_t gx, float dx, float dy,
                                  float inv_m2, int32_t ry, int32_t rx, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Control v1: waypoints -> (throttle, steer, brake) on the device, the step after the sampling loop in the reference's agents
 * (control/controller.py:29-76 `control_pid`, control/pid.py, `post_process_control` of interact.py:218-229 and
 * e2e_driving/diffusion_agent.py:268-277).  One launch per tick for all scenes, no host decision; the PID windows live in
 * device memory and are read and advanced through a pointer, so the call can be a node of a captured graph and a replay
 * carries the windows on.  Callers and fixtures depend on this definition -- a change is a new version, never an edit.
 *
 * Per scene s, all arithmetic in fp32, no contraction, every product, sum, division and square root rounded on its own, in the
 * order written; fixed evaluation order, no atomics.  clip(x, lo, hi) = x < lo ? lo : (x > hi ? hi : x): a NaN goes through.
 * |v| = sqrtf(v.x * v.x + v.y * v.y).
 *
 *   traj      [S][H][D], the model's own units: the clamped result BEFORE xy scaling, the units of selection cost v1.
 *   waypoints wp[i] = (sign_x * (xy_scale * traj[s][i][0]), xy_scale * traj[s][i][1]), i = 0..W-1, 2 <= W <= H; a missing
 *             y column (D = 1) counts as 0.  sign_x = -1 is the callers' `renew_traj`, xy_scale their `model.magic_num`.
 *   target    tgt = (sign_x * (target_scale * target[s][0]), target_scale * target[s][1]); target NULL: waypoint W of the same
 *             trajectory under the waypoint scaling (interact.py's `traj[0, 4, :2]`; needs W < H).
 *   desired   the sum over i = 0..W-2, in index order, of (|wp[i+1] - wp[i]| * 2) / (float)(W - 1).
 *   aim       wp[i*], i* = the smallest i in 0..W-2 that minimises key_i = |aim_dist - |(wp[i+1] + wp[i]) / 2||, among the i
 *             with key_i < |aim_dist - 1e5| (strictly); i* = 0 when none qualifies.  A NaN key never qualifies.  (The
 *             reference's sequential rule -- start from best = 1e5, take i whenever it is strictly closer -- restated.)
 *   heading   heading(v) = (((float)(pi/2) - atan2f(v.y, v.x)) * (float)(180/pi)) / 90:  a = heading(aim),
 *             a_last = heading(wp[W-1] - wp[W-2]), a_t = heading(tgt).
 *   to_target |a_t| < |a|  or  (|a_t - a_last| > angle_thresh and tgt.y < dist_thresh).
 *   steer     clip(PID_turn(to_target ? a_t : a), -1, 1).
 *   brake     desired < brake_speed  or  speed / desired > brake_ratio, speed = velocity[s].
 *   throttle  delta = clip(desired - speed, 0, clip_delta); r = PID_speed(delta) (stepped on every tick, braking or not);
 *             throttle = brake ? 0 : clip(r, 0, max_throttle).
 *   PID(e)    the window holds the last n samples, oldest first c_0 .. c_{n-1} with c_{n-1} = e, and starts as n zeros;
 *             previous = c_{n-2}.  n >= 2: (k_p * e + k_i * mean) + k_d * (e - previous).  n = 1: k_p * e (control/pid.py: a
 *             window of one sample has zero I and D terms).
 *   mean      p_l = c_l + c_{l+64} + c_{l+128} + c_{l+192} (left to right, the j < n only; no such j: +0) for l = 0..63, then six
 *             rounds p_l = p_l + p_{l ^ off}, off = 32, 16, 8, 4, 2, 1, and mean = p_0 / (float)n.
 *   post      0: none.  1 (e2e agent): brake < 0.05f -> brake = 0; throttle > brake -> brake = 0; brake > 0.5f -> throttle = 0.
 *             2 (interact.py): the same two first rules; brake > 0.5f -> brake = 1, steer = 0, throttle = 0.
 *   source    0: the PID path above.  1: the callers' D > 2 path, (throttle, steer, brake) = post(traj[s][0][D-3..D-1]) bit for
 *             bit; it touches no PID state and needs D >= 3.
 *   control   [S][3] = (throttle, steer, brake); brake is 0.0 or 1.0 on the PID path.
 *   state     one device buffer of adx_control_state_bytes(scenes, n_turn, n_speed) bytes, opaque to callers, all zero bytes =
 *             fresh windows.  It holds both windows and their ring positions per scene; every launch reads and advances it
 *             through the pointer -- nothing about it is a by-value argument.  (Today: per scene 2 + n_turn + n_speed 32-bit
 *             words = the two next-slot indices, the turn ring, the speed ring; an index is taken modulo its ring's length.)
 *   rounding  the controls are defined up to fp32 rounding of the operations above and the accuracy of atan2f
 *             (tests/control_ref.py restates them in fp64 and derives the bound); the three decisions -- i*, to_target, brake --
 *             exactly wherever their margins exceed that rounding.  A scene's result does not depend on the other scenes of
 *             the launch, and the same input and state give the same bits on every launch.
 *
 * ADX_ERR_INVALID before any GPU work: W outside 2..H, H outside 2..64, D outside 1..16, source = 1 with D < 3, source or post
 * not one of the above, a NULL target with W = H, a window length outside 1..256, scenes outside 1..65535, a NULL pointer
 * other than target (step) or mask (reset), control or the state overlapping an input or each other.
 * -----------------------------------------------------------------------------------*/
#define ADX_CONTROL_SOURCE_PID 0
#define ADX_CONTROL_SOURCE_ACTION 1
#define ADX_CONTROL_POST_NONE 0
#define ADX_CONTROL_POST_AGENT 1
#define ADX_CONTROL_POST_INTERACT 2
#define ADX_CONTROL_MAX_WINDOW 256
typedef struct adx_control_cfg {
  int32_t scenes, horizon, dim, waypoints, n_turn, n_speed, source, post;
  float sign_x, xy_scale, target_scale;
  float turn_kp, turn_ki, turn_kd, speed_kp, speed_ki, speed_kd;
  float aim_dist, angle_thresh, dist_thresh, brake_speed, brake_ratio, clip_delta, max_throttle;
} adx_control_cfg;
size_t adx_control_state_bytes(int32_t scenes, int32_t n_turn, int32_t n_speed);   /* 0 for a value out of range */
/* traj [scenes][H][D]; velocity [scenes]; target [scenes][2] or NULL; state as above; control [scenes][3]. */
int adx_control_step(const adx_control_cfg* c, const float* traj, const float* velocity, const float* target, void* state,
                     float* control, adx_stream s);
/* Fresh windows for the scenes with mask[s] != 0 (mask: [scenes] bytes on the device, NULL = every scene); a capturable launch. */
int adx_control_reset(void* state, int32_t scenes, int32_t n_turn, int32_t n_speed, const uint8_t* mask, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Stop-short fallback v1: re-time a plan so that it brakes to a halt before its first conflicting waypoint.  The deterministic
 * last resort of a sampling planner: the guide pushes samples away from obstacles and a hard selection prefers a free candidate,
 * but neither promises that the plan a tick ends with is free.  This launch keeps the GEOMETRY of that plan -- every output
 * waypoint lies on the input's polyline before the conflict -- and changes its SPEED PROFILE; control v1 takes its desired
 * speed from the spacing of the first waypoints, so a re-timed plan brakes through the controller as it is.  One launch for all
 * rows, no host decision, no allocation, no synchronisation: a node of a captured graph between selection and control.  No
 * reference counterpart.  Callers and fixtures depend on this definition -- a change is a new version, never an edit.
 *
 *   traj, out  float32 [rows][H][D] in the model's own units (the clamped result before xy scaling, the units of selection
 *              and control), 1 <= H <= 64, D >= 2.  out == traj (the same pointer) is allowed: the wave that owns a row reads
 *              all of it before it writes.
 *   guide ..   the records of cost guidance v1 / v2 / v4 / v5, as adx_guide_cost_capsule takes them; row r reads scene
 *              r % scene_rows.  Motion limits (v3) are not places and take no part: there is no such argument.  iters, lambda
 *              and cap are not read.
 *   params     float32 [param_rows][2] = (gap, decel) in device memory, read at every launch; row r reads r % param_rows.
 *              gap: the arc length to keep before the conflict.  decel: the most a step's length may shrink per waypoint.
 *
 * All arithmetic is fp32, no contraction; every +, -, *, /, sqrtf and compare below is one correctly rounded operation, in the
 * order written.  Per row, with p_h = (x_h, y_h) = traj[r][h][0..1]:
 *
 *   conflict   waypoint h conflicts when the `active` count of cost guidance's waypoint routine (discs at time h, planes,
 *              field, route, capsules -- exactly what adx_guide_cost_capsule counts for that waypoint without motion limits) is
 *              > 0, or when x_h or y_h is not finite (a NaN compares false against every constraint and must not pass as free).
 *   first      the lowest conflicting h, or H when there is none.
 *   free row   first == H:  out row = traj row bit for bit (all D columns), status = 0, stop_at = +inf, active_after = 0.
 *   arc        seg_0 = 0;  seg_h = sqrtf(dx * dx + dy * dy), (dx, dy) = p_h - p_{h-1}, for 1 <= h < first;  seg_h = 0 for
 *              h >= first: nothing at or beyond the conflict is read as geometry.  s_0 = 0, s_h = s_{h-1} + seg_h, summed in
 *              index order (so that q_h == s_h bit for bit while the plan's own speed governs).
 *   stop       g = gap >= 0 ? gap : 0 (a NaN gives 0).  first >= 1: t = s_{first-1} - g, L = t > 0 ? t : 0.  first == 0: L = 0.
 *              stop_at = L.
 *   profile    q_0 = 0.  For h = 1 .. H-1 in order:  d = L - q_{h-1};  w = h < first ? seg_h : +inf;  u = d < w ? d : w;
 *              when decel is finite and >= 0 (a = decel; otherwise the limit is off, as inf is in the motion limits):
 *              e = (sqrtf(a * a + (8 * a) * d) - a) * 0.5 and u = e < u ? e : u;  then u_h = u, q_h = q_{h-1} + u.
 *              e(d) is the step length from which a body that sheds `a` per step still stops within d: e(d - u) = u - a when
 *              u = e(d).  A binding envelope sheds exactly decel per step; only the last approach, which lands on L through
 *              d, may shed more.  decel = 0: do not move.
 *   status     2 when H > 1, first > 1, the limit is on and seg_1 - u_1 > a: the first step already has to shed more than the
 *              limit, the plan cannot stop in time and a consumer may want full brake.  Otherwise 1 (0: a free row).
 *   resample   j = the largest k in 0 .. first-1 with s_k <= q_h.  first == 0: out_h = p_0.  j == first - 1 or q_h == s_j:
 *              out_h = p_j, a select and not an addition (the sign of a zero survives).  Otherwise
 *              t = (q_h - s_j) / (s_{j+1} - s_j) and out_h = p_j + t * (p_{j+1} - p_j) per component.  Columns >= 2 of row
 *              h are traj's, unchanged.  out_0 == p_0 in bits; while the plan's own speed governs, out_h == p_h in bits.
 *   residual   active_after = the active count of the out row under the same records: the lane evaluation and butterfly of
 *              adx_guide_cost.  It is NOT promised to be 0: the launch looks at waypoints only, as the guide does, and a moving
 *              obstacle can reach a stopped ego.  The caller gets the number instead of a promise.
 *   outputs    first, status, active_after int32 [rows]; stop_at float32 [rows].
 *
 * ADX_ERR_INVALID before any GPU work, each with its own text: a NULL traj, out, params or output; NULL guide and NULL field;
 * horizon outside 1..64; dim < 2; param_rows < 1; an empty shape or one beyond the 32-bit element index; whatever cost guidance
 * v1, v2, v4 and v5 refuse of their records; records without a point-wise term (no discs, planes, field, route or capsules); an
 * output overlapping traj, params, a record's array or another output, except out == traj.
 * -----------------------------------------------------------------------------------*/
int adx_stop_short(const float* traj, const adx_guide* guide, const adx_guide_field* field, const adx_guide_route* route,
                   const adx_guide_capsules* capsules, const float* params /* [param_rows][2] = (gap, decel) */, int32_t param_rows,
                   float* out, int32_t* first, int32_t* status, float* stop_at, int32_t* active_after, int32_t rows,
                   int32_t horizon, int32_t dim, adx_stream s);

/* ------------------------------------------------------------------------------------
 * Open-loop metrics v1: how far sampled plans lie from logged waypoints -- ADE / FDE of the chosen plan, minADE_K / minFDE_K
 * over a scene's candidates, miss flags, the chosen plan's displacement per waypoint and its final error split along and across
 * the logged heading.  One launch per batch (adx_traj_metrics) and one launch that folds the batch into a device-resident state
 * (adx_metrics_accumulate): no host decision, no allocation, no synchronisation, so both can follow a captured tick.  No
 * reference counterpart: the reference's train.evaluate paints dots (train.py:62-90).  Callers and fixtures depend on this
 * definition -- a change is a new version, never an edit.
 *
 *   trajs     float32 [K * S][H][D], candidate-major as adx_traj_select takes them: candidate k of scene s is row k * S + s.
 *             1 <= K <= 64, 1 <= H <= 64, D >= 2; columns 0, 1 are (x, y) in the model's own units.
 *   gt        float32 [S][H][2], the logged waypoints in the units of trajs.
 *   valid     int32 [S] or NULL: n_s, how many of the scene's logged waypoints count, clamped to [0, H]; NULL: H.
 *   index     int32 [S] or NULL: the chosen candidate (adx_traj_select's index); NULL: candidate 0.  A value outside [0, K)
 *             makes the scene unscored; it is compared, never used as an address.
 *   cfg       h0: the first scored waypoint (callers pass 1: waypoint 0 is the ego pose the sampling loops zero); waypoints
 *             h0 <= h < n_s are scored.  xy_scale: metres per model unit (model.magic_num).  miss_radius: metres.
 *
 * A scene is scored when n_s > h0 and its index is in range.  An unscored scene writes zeros to every output, flags 0.  All
 * arithmetic is fp32, no contraction; every +, -, *, / and sqrtf below is one correctly rounded operation, in the order written.
 * Per scored scene, with n = n_s:
 *
 *   disp      per candidate k and scored h: ex = (x - gx) * xy_scale, ey = (y - gy) * xy_scale, disp_h = sqrtf(ex * ex + ey * ey);
 *             disp_h = 0 for every other h < 64.
 *   ade[s][k] p_l = disp_l for l = 0..63, then six rounds p_l = p_l + p_{l ^ off}, off = 32, 16, 8, 4, 2, 1, and
 *             ade = p_0 / (float)(n - h0).
 *   fde[s][k] disp_{n-1}.
 *   search    argmin(v): the smallest k among the smallest finite v_k; no finite v_k: 0 (ties to the lowest k, a non-finite
 *             value loses to every finite one: the rule of selection cost v1).
 *   best[s]   argmin(ade).
 *   rec[s]    8 floats: min_ade = ade[best], min_fde = fde[argmin(fde)] (its own search), sel_ade = ade[index],
 *             sel_fde = fde[index], along, cross, miss_sel = sel_fde > miss_radius ? 1 : 0, miss_any = min_fde > miss_radius ? 1 : 0
 *             (a NaN is not a miss; bit 2 of the flags tells).
 *   heading   d = gt[n-1] - gt[n-2] (model units), len = sqrtf(d.x * d.x + d.y * d.y); valid when n - h0 >= 2 and
 *             0 < len < inf.  u = (d.x / len, d.y / len); with (ex, ey) the chosen candidate's error at h = n - 1:
 *             along = ex * u.x + ey * u.y (longitudinal), cross = ey * u.x - ex * u.y (lateral, left positive).  Not valid: both 0.
 *   flags[s]  bit 0: scored.  bit 1: heading valid.  bit 2: sel_ade is finite (every scored disp of the chosen candidate is
 *             finite and so is their sum).  Bits 8..14: n.  Bits 16..22: h0.  (The upper fields let the accumulation know the
 *             scored range of disp_sel without a second look at valid.)
 *   disp_sel  [S][H]: the chosen candidate's disp_h, 0 outside the scored range.
 *   rounding  the float outputs are defined up to fp32 rounding of the operations above (tests/metrics_ref.py restates them in
 *             fp64 and derives the bound); best and the miss fields exactly wherever their margins exceed that rounding.  A
 *             scene's result does not depend on the other scenes of the launch; no atomics, fixed trees: the same input
 *             gives the same bits on every launch.
 *
 * Accumulation.  The state is one device buffer of adx_metrics_state_bytes() bytes, opaque to callers, all zero bytes = empty
 * (today 144 8-byte words: int64 counts and fp64 sums).  adx_metrics_accumulate walks the scenes of one batch in index order, each
 * statistic in fp64 on a thread of its own (one workgroup), so the state's bits depend on the batches and their order alone:
 *   words 0..4    int64: scenes scored; of those, scenes whose chosen plan is not finite (bit 2 clear) -- counted here and left
 *                 out of everything below; heading-valid scenes; scenes with best == index (index NULL: 0); scenes with
 *                 blocked != 0 (blocked NULL: none)
 *   words 5..12   fp64 sums of rec[0..7]
 *   word 13       fp64 sum of (double)sel_ade - (double)min_ade, the selector's regret
 *   words 14, 15  fp64 sums of |along| and |cross| over the heading-valid scenes
 *   words 16+h    fp64 sum of disp_sel[s][h] over the scenes with h0 <= h < n;  words 80+h: int64, how many those are
 *
 * ADX_ERR_INVALID before any GPU work, each with its own text: a NULL configuration or required pointer; candidates or horizon
 * outside 1..64, dim < 2, scenes outside 1..65535; h0 outside 0..horizon-1; xy_scale not finite or not > 0; miss_radius negative
 * or NaN; an output overlapping an input or another output; K * S * H * D above 0x3fffffff.  Accumulate and reset: a NULL
 * pointer other than index and blocked, scenes or horizon out of range, the state overlapping an input.
 * -----------------------------------------------------------------------------------*/
#define ADX_METRICS_REC 8
#define ADX_METRICS_FLAG_SCORED 1
#define ADX_METRICS_FLAG_HEADING 2
#define ADX_METRICS_FLAG_FINITE 4
typedef struct adx_metrics_cfg {
  int32_t scenes, candidates, horizon, dim, h0;
  float miss_radius, xy_scale;
} adx_metrics_cfg;
/* trajs, gt, valid, index as above; ade, fde float32 [scenes][candidates]; best int32 [scenes]; rec float32 [scenes][8];
 * flags int32 [scenes]; disp_sel float32 [scenes][horizon]. */
int adx_traj_metrics(const adx_metrics_cfg* c, const float* trajs, const float* gt, const int32_t* valid, const int32_t* index,
                     float* ade, float* fde, int32_t* best, float* rec, int32_t* flags, float* disp_sel, adx_stream s);
size_t adx_metrics_state_bytes(void);
/* An empty state; a capturable launch. */
int adx_metrics_reset(void* state, adx_stream s);
/* rec, flags, best, disp_sel: one adx_traj_metrics launch's outputs; index: what that launch was given (or NULL); blocked int32
 * [scenes] or NULL: 1 where the chosen plan still violates the guide (selection cost v2's `blocked`, or active > 0). */
int adx_metrics_accumulate(void* state, const float* rec, const int32_t* flags, const int32_t* best, const int32_t* index,
                           const float* disp_sel, const int32_t* blocked, int32_t scenes, int32_t horizon, adx_stream s);

/* add_noise (train.py:234) fused with the [...,0,:3] = 0 of train.py:235 when zero_first != 0.
 * sqrt_ab / sqrt_1mab are the host tables sqrt(abar), sqrt(1-abar) of length n_train.  Refused: batch * horizon * dim above
 * 0x3fffffff, more elements than the kernel's 32-bit index holds. */
int adx_add_noise(const float* x, const float* noise, const int64_t* t, const float* sqrt_ab, const float* sqrt_1mab,
                  int32_t n_train, float* out, int32_t batch, int32_t horizon, int32_t dim, int32_t zero_first,
                  adx_stream s);

/* Camera front-end (interact.py:73-78, e2e_driving/diffusion_agent.py:96-101): ToTensor + Normalize of uint8
 * [n][h][w][3] frames into fp32 [n][3][h][w]; mean/std are HOST pointers to 3 floats. */
int adx_image_normalize(const uint8_t* frame_hwc, float* out_nchw, int32_t n, int32_t h, int32_t w, const float* mean,
                        const float* stdv, adx_stream s);

/* Batch image augmentation on the GPU: stand-in for the reference's imgaug pipeline (dataset/augment.py:10-77, applied per
 * sample in dataset/carla_dataset.py:24-31).  frames_hwc: uint8 [n][h][w][3], augmented IN PLACE; scratch: n*h*w*3 bytes
 * (needed when any_blur != 0).  The host draws the plan (autonomous_driving_with_diffusion_model_amd/dataset/augment.py):
 * plan [n][7][8] floats = per image seven operator slots in application order (row = code, p0..p3, per_channel, 0, 0;
 * codes in csrc/augment.hip), seeds [n] for the per-pixel hash randomness, ranges [n][4] = the slot ranges applied before
 * and after the image's blur, blur_sigma [n] (0 = no blur).  All four arrays live on the device. */
int adx_image_augment(uint8_t* frames_hwc, uint8_t* scratch, int32_t n, int32_t h, int32_t w, const float* plan,
                      const uint64_t* seeds, const int32_t* ranges, const float* blur_sigma, int32_t any_blur, adx_stream s);

/* Measurement probe (bench.py's `roofline.sustained`; no reference counterpart): `workgroups` x 4 waves run `iters` trips of
 * the 3x3 convolution's inner loop -- 8 LDS operand reads per 12 v_mfma_f32_32x32x16_f16 -- on the 64 KB of fp16 operand cells
 * at `operands` (device memory), with no global traffic, staging or epilogue: the fp16 MFMA rate the chip sustains at its
 * power limit.  out: workgroups * 256 floats (a checksum, so that nothing is optimised away); *flops (host, optional)
 * receives the MFMA flops of the launch. */
int adx_probe_mfma_fp16(const void* operands, float* out, int32_t workgroups, int32_t iters, double* flops, adx_stream s);
/* The same probe on v_mfma_f32_16x16x32_f16 (the loop of csrc/conv2d_hs16.hip: 16 operand reads per 48 MFMAs -- the same flops and
 * LDS reads per trip).  At the power limit the two shapes sustain different clocks; `roofline.sustained` reports both. */
int adx_probe_mfma_fp16_16x16x32(const void* operands, float* out, int32_t workgroups, int32_t iters, double* flops, adx_stream s);

#ifdef __cplusplus
}
#endif
#endif /* ADX_H */
