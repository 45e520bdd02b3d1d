// extern "C" surface of libadx.so (declared in include/adx.h): thin wrappers over the adx::
// implementations plus the thread-local error string.
#include <stdarg.h>
#include <stdlib.h>

#include "sched.h"
#include "tconv.h"

namespace adx {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

static thread_local PlanSink* t_plan_sink = nullptr;
PlanSink* plan_sink() { return t_plan_sink; }
void plan_set_sink(PlanSink* s) { t_plan_sink = s; }

int plan_emit(PlanSink* s, const PlanLaunch& l) {
  ADX_REQUIRE(s->n < s->cap, "plan export: more than %d launches", s->cap);
  s->rec[s->n++] = l;
  return ADX_OK;
}

void plan_write(const PlanLaunch& l, const int layer[5], long long part_off, int32_t* o) {
  const int row_tiles = l.bt > 0 ? (l.rows + l.bt - 1) / l.bt : 0;
  const int32_t v[ADX_PLAN_INTS] = {layer[0], layer[1], layer[2], l.family, l.bt, row_tiles, l.bt > 0 ? l.rows % l.bt : 0, l.ctiles,
                                    l.grid, l.ksplit, l.reduce, l.chunks, l.vec_stage, l.fast_epi, l.ntap, layer[3], layer[4],
                                    l.ctiles_b, l.ck, l.cin_pad, (int32_t)l.part_floats, (int32_t)part_off, (int32_t)l.lds_bytes,
                                    l.lout, l.cout, l.aux, 0, 0};
  for (int i = 0; i < ADX_PLAN_INTS; ++i) o[i] = v[i];
}

const DebugSwitches& debug_switches() {
  static const DebugSwitches sw = [] {
    DebugSwitches d;
    // exact one-character values: "10" is not "1" (the Python side compares whole strings too)
    auto is = [](const char* name, char v) { const char* e = getenv(name); return e != nullptr && e[0] == v && e[1] == '\0'; };
    d.conv_exact = is("ADX_CONV_EXACT", '1');
    d.wgrad_exact = is("ADX_WGRAD_EXACT", '1');
    d.tconv_exact = is("ADX_TCONV_EXACT", '1');
    d.unet_chain = !is("ADX_UNET_CHAIN", '0');
    d.unet_pipe = !is("ADX_UNET_PIPE", '0');
    d.conv_cells = !is("ADX_CONV_CELLS", '0');
    d.conv_vrow = !is("ADX_CONV_VROW", '0');
    d.train_cells = is("ADX_TRAIN_CELLS", '0') ? 0 : (is("ADX_TRAIN_CELLS", '1') ? 1 : (is("ADX_TRAIN_CELLS", '2') ? 2 : (is("ADX_TRAIN_CELLS", '3') ? 3 : (is("ADX_TRAIN_CELLS", '4') ? 4 : 5))));
    d.check_range = is("ADX_CHECK_RANGE", '1');
    d.hs_dma = !is("ADX_HS_DMA", '0');
    d.hs_persist = !is("ADX_HS_PERSIST", '0');
    d.hs_pair = !is("ADX_HS_PAIR", '0');
    d.hs_s2q = !is("ADX_HS_S2Q", '0');
    d.wgrad_deterministic = is("ADX_WGRAD_DETERMINISTIC", '1');
    if (const char* e = getenv("ADX_CHAIN_MASK")) d.chain_mask = (unsigned)strtoul(e, nullptr, 0);
    if (const char* e = getenv("ADX_HS_MODE")) d.hs_mode = atoi(e);
    if (const char* e = getenv("ADX_HS_RESERVE_CUS")) d.hs_reserve_cus = atoi(e) < 0 ? 0 : (atoi(e) & ~7);
    if (const char* e = getenv("ADX_HS_GRID_CAP")) d.hs_grid_cap = atoi(e) < 8 ? 0 : (atoi(e) & ~7);
    if (const char* e = getenv("ADX_RESNET_SPLIT_FROM")) d.resnet_split_from = atoi(e) < 0 ? -1 : atoi(e);
    if (const char* e = getenv("ADX_RESNET_STREAMS")) d.resnet_streams = atoi(e) < 1 ? 1 : (atoi(e) > 4 ? 4 : atoi(e));
    return d;
  }();
  return sw;
}

int embed_forward(const adx_embed_weights* w, int dim, const int64_t* t, int t_rows, const float* cond,
                  const float* feat, int feat_rows, int rows, float* time_embed, float* mish_cond, hipStream_t s);
size_t control_state_bytes(int scenes, int n_turn, int n_speed);
int control_step(const adx_control_cfg* c, const float* traj, const float* velocity, const float* target, void* state,
                 float* control, hipStream_t s);
int control_reset(void* state, int scenes, int n_turn, int n_speed, const uint8_t* mask, hipStream_t s);

// The step exports: each names its schedule, its noise source, its pin and its guide records; these two fill the one record of
// sched.h, and step_run / dpm_run check it and pick the kernel instantiation.  The order every call below keeps: the schedule, the
// model output and the sample, then the noise (z: a tensor, or ns, slot, row_offset: a state), then tgt and mask (the inpainting
// blend; step only), the pin, the records, the two outputs and the shape.  Adjacent pointers of one type are (z, ns), (tgt, mask)
// and (prev, x0); each family of exports below names which of them it leaves null.
static int step(bool ddpm, const adx_step_coef* c, const float* mo, const float* x, const float* z, const uint32_t* ns, int32_t slot,
                int64_t row_offset, const float* tgt, const float* mask, const adx_pin* pin, const GuideRecords& g, float* prev, float* x0,
                int batch, int horizon, int dim, adx_stream s) {
  StepCall k;
  k.ddpm = ddpm; k.c = c; k.mo = mo; k.x = x; k.z = z; k.ns = ns; k.slot = slot; k.row_offset = row_offset; k.tgt = tgt; k.mask = mask;
  k.pin = pin; k.g = g; k.prev = prev; k.x0 = x0; k.batch = batch; k.horizon = horizon; k.dim = dim; k.stream = (hipStream_t)s;
  return step_run(k);
}
static int dpm(const adx_dpm_coef* c, const float* mo, const float* x, const float* px0, const uint32_t* ns, int32_t slot,
               int64_t row_offset, const adx_pin* pin, const GuideRecords& g, float* prev, float* x0, int batch, int horizon, int dim,
               adx_stream s) {
  DpmCall k;
  k.c = c; k.mo = mo; k.x = x; k.px0 = px0; k.ns = ns; k.slot = slot; k.row_offset = row_offset; k.pin = pin; k.g = g; k.prev = prev;
  k.x0 = x0; k.batch = batch; k.horizon = horizon; k.dim = dim; k.stream = (hipStream_t)s;
  return dpm_run(k);
}
}  // namespace adx

extern "C" {

#ifndef ADX_SRC_HASH
#define ADX_SRC_HASH "unknown"
#endif
int adx_version(void) { return 2; }
// the "ADX_SRC_HASH=" tag lets a build script read the hash out of the file without loading the library
static const char kSrcHash[] = "ADX_SRC_HASH=" ADX_SRC_HASH;
const char* adx_source_hash(void) { return kSrcHash + 13; }
const char* adx_last_error(void) { return adx::g_err; }

size_t adx_tconv_packed_bytes(const adx_tconv_desc* d) {
  if (d == nullptr || adx::tconv_check(d) != ADX_OK) return 0;
  return adx::tconv_packed_floats(d) * sizeof(float);
}
int adx_tconv_pack(const adx_tconv_desc* d, const float* w, float* packed, adx_stream s) {
  return adx::tconv_pack(d, w, packed, (hipStream_t)s);
}
int adx_tconv_forward(const adx_tconv_desc* d, const adx_tconv_io* io, adx_stream s) {
  return adx::tconv_forward(d, io, (hipStream_t)s);
}
int adx_tconv_plan_describe(const adx_tconv_desc* d, int32_t batch, int64_t scratch_floats, int32_t has_tickets, int32_t* n_records,
                            int32_t* ints, int32_t max_records) {
  ADX_REQUIRE(d != nullptr && n_records != nullptr && ints != nullptr, "adx_tconv_plan_describe: null argument");
  ADX_REQUIRE(batch >= 1 && max_records >= 1, "adx_tconv_plan_describe: batch and max_records must be >= 1");
  ADX_REQUIRE(scratch_floats >= 0 && (scratch_floats > 0 || has_tickets == 0), "adx_tconv_plan_describe: ticket words come with a scratch only");
  // placeholder addresses (never read): dense 16-byte aligned tensors, as ops.tconv passes them
  float* const fake = reinterpret_cast<float*>((uintptr_t)1 << 32);
  adx_tconv_io io;
  memset(&io, 0, sizeof(io));
  io.x0 = fake; io.x0_sb = (int64_t)d->c0 * d->lin; io.x0_sc = d->lin; io.x0_sl = 1;
  if (d->c1 > 0) { io.x1 = fake; io.x1_sb = (int64_t)d->c1 * d->lin; io.x1_sc = d->lin; io.x1_sl = 1; }
  io.packed_w = fake; io.bias = fake;
  if (d->groups > 0) { io.gamma = fake; io.beta = fake; }
  io.y = fake; io.y_sb = (int64_t)d->cout * d->lout; io.y_sc = d->lout; io.y_sl = 1;
  io.batch = batch;
  if (scratch_floats > 0) {
    io.scratch = fake; io.scratch_floats = scratch_floats;
    if (has_tickets != 0) io.tickets = reinterpret_cast<uint32_t*>(fake);
  }
  adx::PlanLaunch rec[4];
  adx::PlanSink sink;
  sink.rec = rec; sink.cap = 4;
  int rc;
  {
    adx::PlanScope scope(&sink);
    rc = adx::tconv_forward(d, &io, nullptr);
  }
  if (rc != ADX_OK) return rc;
  ADX_REQUIRE(sink.n <= max_records, "adx_tconv_plan_describe: %d launches, room for %d", sink.n, max_records);
  const int layer[5] = {0, -1, 0, -1, -1};
  for (int i = 0; i < sink.n; ++i) adx::plan_write(rec[i], layer, rec[i].part != nullptr ? 0 : -1, ints + (size_t)i * ADX_PLAN_INTS);
  *n_records = sink.n;
  return ADX_OK;
}
int adx_embed_forward(const adx_embed_weights* w, int32_t dim, const int64_t* t, int32_t t_rows, const float* cond,
                      const float* img_feature, int32_t feat_rows, int32_t rows, float* time_embed, float* mish_cond,
                      adx_stream s) {
  return adx::embed_forward(w, dim, t, t_rows, cond, img_feature, feat_rows, rows, time_embed, mish_cond,
                            (hipStream_t)s);
}
// The plain, _rng and _pin exports: no guide records.  Plain: z alone, tgt and mask, no pin.  _rng: ns alone (refused when null),
// tgt and mask, no pin.  _pin: z and ns as the caller gives them (step_run refuses both at once), no tgt and mask, the pin.
int adx_ddim_step(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                  const float* target, const float* mask, float* prev, float* x0, int32_t batch, int32_t horizon,
                  int32_t dim, adx_stream s) {
  return adx::step(false, c, model_output, sample, noise, nullptr, 0, 0, target, mask, nullptr, {}, prev, x0, batch, horizon, dim, s);
}
int adx_ddpm_step(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                  const float* target, const float* mask, float* prev, float* x0, int32_t batch, int32_t horizon,
                  int32_t dim, adx_stream s) {
  return adx::step(true, c, model_output, sample, noise, nullptr, 0, 0, target, mask, nullptr, {}, prev, x0, batch, horizon, dim, s);
}
int adx_ddim_step_rng(const adx_step_coef* c, const float* model_output, const float* sample, const uint32_t* noise_state,
                      int32_t slot, int64_t row_offset, const float* target, const float* mask, float* prev, float* x0,
                      int32_t batch, int32_t horizon, int32_t dim, adx_stream s) {
  ADX_REQUIRE(noise_state != nullptr, "scheduler step: null noise state");      // to step_run, no state is the tensor path
  return adx::step(false, c, model_output, sample, nullptr, noise_state, slot, row_offset, target, mask, nullptr, {}, prev, x0, batch,
                   horizon, dim, s);
}
int adx_ddpm_step_rng(const adx_step_coef* c, const float* model_output, const float* sample, const uint32_t* noise_state,
                      int32_t slot, int64_t row_offset, const float* target, const float* mask, float* prev, float* x0,
                      int32_t batch, int32_t horizon, int32_t dim, adx_stream s) {
  ADX_REQUIRE(noise_state != nullptr, "scheduler step: null noise state");      // to step_run, no state is the tensor path
  return adx::step(true, c, model_output, sample, nullptr, noise_state, slot, row_offset, target, mask, nullptr, {}, prev, x0, batch,
                   horizon, dim, s);
}
int adx_dpm_step(const adx_dpm_coef* c, const float* model_output, const float* sample, const float* prev_x0,
                 float* prev_sample, float* x0, int32_t batch, int32_t horizon, int32_t dim, adx_stream s) {
  return adx::dpm(c, model_output, sample, prev_x0, nullptr, 0, 0, nullptr, {}, prev_sample, x0, batch, horizon, dim, s);
}
int adx_ddim_step_pin(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                      const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, float* prev, float* x0,
                      int32_t batch, int32_t horizon, int32_t dim, adx_stream s) {
  return adx::step(false, c, model_output, sample, noise, noise_state, slot, row_offset, nullptr, nullptr, pin, {}, prev, x0, batch,
                   horizon, dim, s);
}
int adx_ddpm_step_pin(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                      const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, float* prev, float* x0,
                      int32_t batch, int32_t horizon, int32_t dim, adx_stream s) {
  return adx::step(true, c, model_output, sample, noise, noise_state, slot, row_offset, nullptr, nullptr, pin, {}, prev, x0, batch,
                   horizon, dim, s);
}
int adx_dpm_step_pin(const adx_dpm_coef* c, const float* model_output, const float* sample, const float* prev_x0,
                     const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, float* prev_sample,
                     float* x0, int32_t batch, int32_t horizon, int32_t dim, adx_stream s) {
  return adx::dpm(c, model_output, sample, prev_x0, noise_state, slot, row_offset, pin, {}, prev_sample, x0, batch, horizon, dim, s);
}
int adx_pin_apply(float* x, const adx_pin* pin, const uint32_t* noise_state, int64_t row_offset, int32_t batch, int32_t horizon,
                  int32_t dim, adx_stream s) {
  return adx::pin_apply(x, pin, noise_state, row_offset, batch, horizon, dim, (hipStream_t)s);
}
int adx_traj_select(const adx_select_cfg* c, const float* trajs, const float* target, float* cost, int32_t* index,
                    float* best, adx_stream s) {
  return adx::traj_select(c, trajs, target, cost, index, best, (hipStream_t)s);
}
// "Cost guidance v1" to "v5": one family of exports per version (_guide, _field, _motion, _route, _capsule), each the one before
// with one more record.  All of them hand their records to the same functions as one GuideRecords; what runs (element-wise or
// row-wise step kernel, which terms of guide_grad) follows from which records are there, not from the export's name.
// Every step export of these families passes what _pin passes (z and ns, no tgt and mask, the pin) and then its records.
int adx_ddim_step_guide(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                        const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                        float* prev, float* x0, int32_t batch, int32_t horizon, int32_t dim, adx_stream s) {
  return adx::step(false, c, model_output, sample, noise, noise_state, slot, row_offset, nullptr, nullptr, pin, {guide}, prev, x0,
                   batch, horizon, dim, s);
}
int adx_ddpm_step_guide(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                        const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                        float* prev, float* x0, int32_t batch, int32_t horizon, int32_t dim, adx_stream s) {
  return adx::step(true, c, model_output, sample, noise, noise_state, slot, row_offset, nullptr, nullptr, pin, {guide}, prev, x0,
                   batch, horizon, dim, s);
}
int adx_dpm_step_guide(const adx_dpm_coef* c, const float* model_output, const float* sample, const float* prev_x0,
                       const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                       float* prev_sample, float* x0, int32_t batch, int32_t horizon, int32_t dim, adx_stream s) {
  return adx::dpm(c, model_output, sample, prev_x0, noise_state, slot, row_offset, pin, {guide}, prev_sample, x0, batch, horizon,
                  dim, s);
}
int adx_guide_cost(const float* traj, const adx_guide* guide, float* cost, int32_t* active, int32_t rows, int32_t horizon,
                   int32_t dim, adx_stream s) {
  return adx::guide_cost(traj, {guide}, cost, active, rows, horizon, dim, (hipStream_t)s);
}
int adx_traj_select_guide(const adx_select_guide_cfg* c, const float* trajs, const float* target, const adx_guide* guide,
                          float* cost, int32_t* active, int32_t* index, int32_t* blocked, float* best, adx_stream s) {
  return adx::traj_select_guide(c, trajs, target, {guide}, cost, active, index, blocked, best, (hipStream_t)s);
}
int adx_ddim_step_field(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                        const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                        const adx_guide_field* field, float* prev, float* x0, int32_t batch, int32_t horizon, int32_t dim,
                        adx_stream s) {
  return adx::step(false, c, model_output, sample, noise, noise_state, slot, row_offset, nullptr, nullptr, pin, {guide, field},
                   prev, x0, batch, horizon, dim, s);
}
int adx_ddpm_step_field(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                        const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                        const adx_guide_field* field, float* prev, float* x0, int32_t batch, int32_t horizon, int32_t dim,
                        adx_stream s) {
  return adx::step(true, c, model_output, sample, noise, noise_state, slot, row_offset, nullptr, nullptr, pin, {guide, field},
                   prev, x0, batch, horizon, dim, s);
}
int adx_dpm_step_field(const adx_dpm_coef* c, const float* model_output, const float* sample, const float* prev_x0,
                       const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                       const adx_guide_field* field, float* prev_sample, float* x0, int32_t batch, int32_t horizon, int32_t dim,
                       adx_stream s) {
  return adx::dpm(c, model_output, sample, prev_x0, noise_state, slot, row_offset, pin, {guide, field}, prev_sample, x0, batch,
                  horizon, dim, s);
}
int adx_guide_cost_field(const float* traj, const adx_guide* guide, const adx_guide_field* field, float* cost, int32_t* active,
                         int32_t rows, int32_t horizon, int32_t dim, adx_stream s) {
  return adx::guide_cost(traj, {guide, field}, cost, active, rows, horizon, dim, (hipStream_t)s);
}
int adx_traj_select_guide_field(const adx_select_guide_cfg* c, const float* trajs, const float* target, const adx_guide* guide,
                                const adx_guide_field* field, float* cost, int32_t* active, int32_t* index, int32_t* blocked,
                                float* best, adx_stream s) {
  return adx::traj_select_guide(c, trajs, target, {guide, field}, cost, active, index, blocked, best, (hipStream_t)s);
}
int adx_ddim_step_motion(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                         const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin,
                         const adx_guide* guide, const adx_guide_field* field, const adx_guide_motion* motion, float* prev,
                         float* x0, int32_t batch, int32_t horizon, int32_t dim, adx_stream s) {
  return adx::step(false, c, model_output, sample, noise, noise_state, slot, row_offset, nullptr, nullptr, pin,
                   {guide, field, motion}, prev, x0, batch, horizon, dim, s);
}
int adx_ddpm_step_motion(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                         const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin,
                         const adx_guide* guide, const adx_guide_field* field, const adx_guide_motion* motion, float* prev,
                         float* x0, int32_t batch, int32_t horizon, int32_t dim, adx_stream s) {
  return adx::step(true, c, model_output, sample, noise, noise_state, slot, row_offset, nullptr, nullptr, pin,
                   {guide, field, motion}, prev, x0, batch, horizon, dim, s);
}
int adx_dpm_step_motion(const adx_dpm_coef* c, const float* model_output, const float* sample, const float* prev_x0,
                        const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                        const adx_guide_field* field, const adx_guide_motion* motion, float* prev_sample, float* x0,
                        int32_t batch, int32_t horizon, int32_t dim, adx_stream s) {
  return adx::dpm(c, model_output, sample, prev_x0, noise_state, slot, row_offset, pin, {guide, field, motion}, prev_sample, x0,
                  batch, horizon, dim, s);
}
int adx_guide_cost_motion(const float* traj, const adx_guide* guide, const adx_guide_field* field, const adx_guide_motion* motion,
                          float* cost, int32_t* active, int32_t rows, int32_t horizon, int32_t dim, adx_stream s) {
  return adx::guide_cost(traj, {guide, field, motion}, cost, active, rows, horizon, dim, (hipStream_t)s);
}
int adx_traj_select_guide_motion(const adx_select_guide_cfg* c, const float* trajs, const float* target, const adx_guide* guide,
                                 const adx_guide_field* field, const adx_guide_motion* motion, float* cost, int32_t* active,
                                 int32_t* index, int32_t* blocked, float* best, adx_stream s) {
  return adx::traj_select_guide(c, trajs, target, {guide, field, motion}, cost, active, index, blocked, best, (hipStream_t)s);
}
int adx_ddim_step_route(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                        const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                        const adx_guide_field* field, const adx_guide_motion* motion, const adx_guide_route* route, float* prev,
                        float* x0, int32_t batch, int32_t horizon, int32_t dim, adx_stream s) {
  return adx::step(false, c, model_output, sample, noise, noise_state, slot, row_offset, nullptr, nullptr, pin,
                   {guide, field, motion, route}, prev, x0, batch, horizon, dim, s);
}
int adx_ddpm_step_route(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                        const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                        const adx_guide_field* field, const adx_guide_motion* motion, const adx_guide_route* route, float* prev,
                        float* x0, int32_t batch, int32_t horizon, int32_t dim, adx_stream s) {
  return adx::step(true, c, model_output, sample, noise, noise_state, slot, row_offset, nullptr, nullptr, pin,
                   {guide, field, motion, route}, prev, x0, batch, horizon, dim, s);
}
int adx_dpm_step_route(const adx_dpm_coef* c, const float* model_output, const float* sample, const float* prev_x0,
                       const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin, const adx_guide* guide,
                       const adx_guide_field* field, const adx_guide_motion* motion, const adx_guide_route* route,
                       float* prev_sample, float* x0, int32_t batch, int32_t horizon, int32_t dim, adx_stream s) {
  return adx::dpm(c, model_output, sample, prev_x0, noise_state, slot, row_offset, pin, {guide, field, motion, route},
                  prev_sample, x0, batch, horizon, dim, s);
}
int adx_guide_cost_route(const float* traj, const adx_guide* guide, const adx_guide_field* field, const adx_guide_motion* motion,
                         const adx_guide_route* route, float* cost, int32_t* active, int32_t rows, int32_t horizon, int32_t dim,
                         adx_stream s) {
  return adx::guide_cost(traj, {guide, field, motion, route}, cost, active, rows, horizon, dim, (hipStream_t)s);
}
int adx_traj_select_guide_route(const adx_select_guide_cfg* c, const float* trajs, const float* target, const adx_guide* guide,
                                const adx_guide_field* field, const adx_guide_motion* motion, const adx_guide_route* route,
                                float* cost, int32_t* active, int32_t* index, int32_t* blocked, float* best, adx_stream s) {
  return adx::traj_select_guide(c, trajs, target, {guide, field, motion, route}, cost, active, index, blocked, best, (hipStream_t)s);
}
int adx_ddim_step_capsule(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                          const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin,
                          const adx_guide* guide, const adx_guide_field* field, const adx_guide_motion* motion,
                          const adx_guide_route* route, const adx_guide_capsules* capsules, float* prev, float* x0, int32_t batch,
                          int32_t horizon, int32_t dim, adx_stream s) {
  return adx::step(false, c, model_output, sample, noise, noise_state, slot, row_offset, nullptr, nullptr, pin,
                   {guide, field, motion, route, capsules}, prev, x0, batch, horizon, dim, s);
}
int adx_ddpm_step_capsule(const adx_step_coef* c, const float* model_output, const float* sample, const float* noise,
                          const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin,
                          const adx_guide* guide, const adx_guide_field* field, const adx_guide_motion* motion,
                          const adx_guide_route* route, const adx_guide_capsules* capsules, float* prev, float* x0, int32_t batch,
                          int32_t horizon, int32_t dim, adx_stream s) {
  return adx::step(true, c, model_output, sample, noise, noise_state, slot, row_offset, nullptr, nullptr, pin,
                   {guide, field, motion, route, capsules}, prev, x0, batch, horizon, dim, s);
}
int adx_dpm_step_capsule(const adx_dpm_coef* c, const float* model_output, const float* sample, const float* prev_x0,
                         const uint32_t* noise_state, int32_t slot, int64_t row_offset, const adx_pin* pin,
                         const adx_guide* guide, const adx_guide_field* field, const adx_guide_motion* motion,
                         const adx_guide_route* route, const adx_guide_capsules* capsules, float* prev_sample, float* x0,
                         int32_t batch, int32_t horizon, int32_t dim, adx_stream s) {
  return adx::dpm(c, model_output, sample, prev_x0, noise_state, slot, row_offset, pin, {guide, field, motion, route, capsules},
                  prev_sample, x0, batch, horizon, dim, s);
}
int adx_guide_cost_capsule(const float* traj, const adx_guide* guide, const adx_guide_field* field,
                           const adx_guide_motion* motion, const adx_guide_route* route, const adx_guide_capsules* capsules,
                           float* cost, int32_t* active, int32_t rows, int32_t horizon, int32_t dim, adx_stream s) {
  return adx::guide_cost(traj, {guide, field, motion, route, capsules}, cost, active, rows, horizon, dim, (hipStream_t)s);
}
int adx_traj_select_guide_capsule(const adx_select_guide_cfg* c, const float* trajs, const float* target, const adx_guide* guide,
                                  const adx_guide_field* field, const adx_guide_motion* motion, const adx_guide_route* route,
                                  const adx_guide_capsules* capsules, float* cost, int32_t* active, int32_t* index,
                                  int32_t* blocked, float* best, adx_stream s) {
  return adx::traj_select_guide(c, trajs, target, {guide, field, motion, route, capsules}, cost, active, index, blocked, best, (hipStream_t)s);
}
int adx_traj_modes(const adx_modes_cfg* c, const float* trajs, float* modes, int32_t* index, int32_t* mass, int32_t* assign,
                   int32_t* count, float* dist2, adx_stream s) {
  return adx::traj_modes(c, trajs, modes, index, mass, assign, count, dist2, (hipStream_t)s);
}
size_t adx_commit_state_bytes(int32_t scenes, int32_t horizon) { return adx::commit_state_bytes(scenes, horizon); }
int adx_commit_reset(void* state, int32_t scenes, int32_t horizon, const uint8_t* mask, adx_stream s) {
  return adx::commit_reset(state, scenes, horizon, mask, (hipStream_t)s);
}
int adx_traj_commit(const adx_commit_cfg* c, const float* trajs, const float* cost, const int32_t* selected, const int32_t* active,
                    const float* motion, void* state, float* best, int32_t* index, int32_t* status, int32_t* follower,
                    int32_t* blocked, float* dist2, adx_stream s) {
  return adx::traj_commit(c, trajs, cost, selected, active, motion, state, best, index, status, follower, blocked, dist2,
                          (hipStream_t)s);
}
size_t adx_nav_state_bytes(int32_t scenes) { return adx::nav_state_bytes(scenes); }
int adx_nav_reset(void* state, int32_t scenes, const uint8_t* mask, adx_stream s) {
  return adx::nav_reset(state, scenes, mask, (hipStream_t)s);
}
int adx_nav_step(const adx_nav_cfg* c, const double* route, const int32_t* cmd, const int32_t* len, const double* pose, void* state,
                 float* target, int32_t* command, float* window, float* motion, int32_t* fresh, int32_t* head_out, adx_stream s) {
  return adx::nav_step(c, route, cmd, len, pose, state, target, command, window, motion, fresh, head_out, (hipStream_t)s);
}
size_t adx_vehicle_state_bytes(int32_t scenes) { return adx::vehicle_state_bytes(scenes); }
int adx_vehicle_reset(void* state, int32_t scenes, const double* pose, const double* speed, const uint8_t* mask, double* pose_out,
                      float* velocity_out, float* yaw_rate_out, adx_stream s) {
  return adx::vehicle_reset(state, scenes, pose, speed, mask, pose_out, velocity_out, yaw_rate_out, (hipStream_t)s);
}
int adx_vehicle_step(const adx_vehicle_cfg* c, const float* control, const int32_t* hold, void* state, double* pose, float* velocity,
                     float* yaw_rate, adx_stream s) {
  return adx::vehicle_step(c, control, hold, state, pose, velocity, yaw_rate, (hipStream_t)s);
}
size_t adx_drive_state_bytes(int32_t scenes) { return adx::drive_state_bytes(scenes); }
int adx_drive_reset(void* state, int32_t scenes, const uint8_t* mask, int32_t* done, adx_stream s) {
  return adx::drive_reset(state, scenes, mask, done, (hipStream_t)s);
}
int adx_drive_step(const adx_drive_cfg* c, const double* pose, const float* velocity, const float* yaw_rate, const double* route,
                   const int32_t* len, const double* cum, const double* discs, const double* boxes, void* state, int32_t* done,
                   adx_stream s) {
  return adx::drive_step(c, pose, velocity, yaw_rate, route, len, cum, discs, boxes, state, done, (hipStream_t)s);
}
size_t adx_signals_state_bytes(int32_t scenes) { return adx::signals_state_bytes(scenes); }
int adx_signals_reset(void* state, int32_t scenes, const uint8_t* mask, float* planes_out, int32_t n_planes, adx_stream s) {
  return adx::signals_reset(state, scenes, mask, planes_out, n_planes, (hipStream_t)s);
}
int adx_signals_step(const adx_signals_cfg* c, const double* signals, const double* pose, const float* velocity, const int32_t* hold,
                     void* state, float* planes, int32_t* phase, adx_stream s) {
  return adx::signals_step(c, signals, pose, velocity, hold, state, planes, phase, (hipStream_t)s);
}
size_t adx_traffic_state_bytes(int32_t scenes, int32_t n_agents) { return adx::traffic_state_bytes(scenes, n_agents); }
int adx_traffic_reset(const adx_traffic_cfg* c, const double* paths, const int32_t* plen, const double* cum, const double* heading,
                      const double* agents, const uint8_t* mask, void* state, double* boxes, int32_t* leader, adx_stream s) {
  return adx::traffic_reset(c, paths, plen, cum, heading, agents, mask, state, boxes, leader, (hipStream_t)s);
}
int adx_traffic_step(const adx_traffic_cfg* c, const double* paths, const int32_t* plen, const double* cum, const double* heading,
                     const double* agents, const double* stops, const int32_t* phase, const double* pose, const float* velocity,
                     const int32_t* hold, void* state, double* boxes, int32_t* leader, adx_stream s) {
  return adx::traffic_step(c, paths, plen, cum, heading, agents, stops, phase, pose, velocity, hold, state, boxes, leader, (hipStream_t)s);
}
size_t adx_camera_prims_bytes(const adx_camera_cfg* c) { return adx::camera_prims_bytes(c); }
void adx_camera_default_palette(uint8_t* palette, uint8_t* shade) { adx::camera_default_palette(palette, shade); }
int adx_camera_render(const adx_camera_cfg* c, const double* pose, const double* boxes, const double* discs, const double* signals,
                      const int32_t* phase, const double* roads, const int32_t* road_len, const int32_t* hold, void* prims,
                      uint8_t* frames, float* image, int32_t* ids, float* depth, adx_stream s) {
  return adx::camera_render(c, pose, boxes, discs, signals, phase, roads, road_len, hold, prims, frames, image, ids, depth, (hipStream_t)s);
}
int adx_expert_plan(const adx_expert_cfg* c, const float* window, const float* velocity, const float* boxes, const float* discs,
                    const float* planes, float* plan, int32_t* leader, float* info, adx_stream s) {
  return adx::expert_plan(c, window, velocity, boxes, discs, planes, plan, leader, info, (hipStream_t)s);
}
int adx_world_to_ego(int32_t kind, const double* in, const double* pose, float* out, int32_t scenes, int32_t n, double xy_scale,
                     double vel_scale, adx_stream s) {
  return adx::world_to_ego(kind, in, pose, out, scenes, n, xy_scale, vel_scale, (hipStream_t)s);
}
int adx_ego_to_world(const float* plans, const double* pose, double* out, int32_t rows, int32_t scenes, int32_t horizon,
                     int32_t dim, double xy_scale, adx_stream s) {
  return adx::ego_to_world(plans, pose, out, rows, scenes, horizon, dim, xy_scale, (hipStream_t)s);
}
int adx_capsules_from_boxes(const float* boxes, float* out, int32_t scenes, int32_t n_boxes, float inflate, adx_stream s) {
  return adx::capsules_from_boxes(boxes, out, scenes, n_boxes, inflate, (hipStream_t)s);
}
int adx_cost_field_from_occupancy(const float* occ, float* cells, int32_t scenes, int32_t gy, int32_t gx, float dx, float dy,
                                  float inv_m2, int32_t ry, int32_t rx, adx_stream s) {
  return adx::field_from_occupancy(occ, cells, scenes, gy, gx, dx, dy, inv_m2, ry, rx, (hipStream_t)s);
}
size_t adx_control_state_bytes(int32_t scenes, int32_t n_turn, int32_t n_speed) {
  return adx::control_state_bytes(scenes, n_turn, n_speed);
}
int adx_control_step(const adx_control_cfg* c, const float* traj, const float* velocity, const float* target, void* state,
                     float* control, adx_stream s) {
  return adx::control_step(c, traj, velocity, target, state, control, (hipStream_t)s);
}
int adx_control_reset(void* state, int32_t scenes, int32_t n_turn, int32_t n_speed, const uint8_t* mask, adx_stream s) {
  return adx::control_reset(state, scenes, n_turn, n_speed, mask, (hipStream_t)s);
}
int adx_traj_metrics(const adx_metrics_cfg* c, const float* trajs, const float* gt, const int32_t* valid, const int32_t* index,
                     float* ade, float* fde, int32_t* best, float* rec, int32_t* flags, float* disp_sel, adx_stream s) {
  return adx::traj_metrics(c, trajs, gt, valid, index, ade, fde, best, rec, flags, disp_sel, (hipStream_t)s);
}
size_t adx_metrics_state_bytes(void) { return adx::metrics_state_bytes(); }
int adx_metrics_reset(void* state, adx_stream s) { return adx::metrics_reset(state, (hipStream_t)s); }
int adx_metrics_accumulate(void* state, const float* rec, const int32_t* flags, const int32_t* best, const int32_t* index,
                           const float* disp_sel, const int32_t* blocked, int32_t scenes, int32_t horizon, adx_stream s) {
  return adx::metrics_accumulate(state, rec, flags, best, index, disp_sel, blocked, scenes, horizon, (hipStream_t)s);
}
int adx_stop_short(const float* traj, const adx_guide* guide, const adx_guide_field* field, const adx_guide_route* route,
                   const adx_guide_capsules* capsules, const float* params, int32_t param_rows, float* out, int32_t* first,
                   int32_t* status, float* stop_at, int32_t* active_after, int32_t rows, int32_t horizon, int32_t dim, adx_stream s) {
  return adx::stop_short(traj, {guide, field, nullptr, route, capsules}, params, param_rows, out, first, status, stop_at, active_after,
                         rows, horizon, dim, (hipStream_t)s);
}
int adx_noise_normal(const uint32_t* state, int32_t slot, int64_t first_elem, float* out, int64_t n, adx_stream s) {
  return adx::noise_normal(state, slot, first_elem, out, n, (hipStream_t)s);
}
int adx_noise_words(const uint32_t* state, int32_t slot, int64_t first_elem, uint32_t* out, int64_t n, adx_stream s) {
  return adx::noise_words(state, slot, first_elem, out, n, (hipStream_t)s);
}
int adx_noise_advance(uint32_t* state, adx_stream s) { return adx::noise_advance(state, (hipStream_t)s); }
int adx_warm_init(const float* prev, int32_t prev_rows, const float* motion, float* out, int32_t rows, int32_t horizon,
                  int32_t dim, int32_t shift, float sqrt_ab, float sqrt_1mab, const uint32_t* noise_state, int64_t row_offset,
                  int32_t zero_first, adx_stream s) {
  return adx::warm_init(prev, prev_rows, motion, out, rows, horizon, dim, shift, sqrt_ab, sqrt_1mab, noise_state, row_offset,
                        zero_first, (hipStream_t)s);
}
int adx_add_noise(const float* x, const float* noise, const int64_t* t, const float* sqrt_ab, const float* sqrt_1mab,
                  int32_t n_train, float* out, int32_t batch, int32_t horizon, int32_t dim, int32_t zero_first,
                  adx_stream s) {
  return adx::add_noise(x, noise, t, sqrt_ab, sqrt_1mab, n_train, out, batch, horizon, dim, zero_first, (hipStream_t)s);
}

int adx_image_normalize(const uint8_t* frame_hwc, float* out_nchw, int32_t n, int32_t h, int32_t w, const float* mean,
                        const float* stdv, adx_stream s) {
  return adx::image_normalize(frame_hwc, out_nchw, n, h, w, mean, stdv, (hipStream_t)s);
}

}  // extern "C"
