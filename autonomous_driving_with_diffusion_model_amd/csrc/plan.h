// The plan export (include/adx.h: adx_unet_plan_describe, adx_tconv_plan_describe): a recorder the launch functions of the
// temporal stack hand their finished argument block to INSTEAD of launching.  The describe calls run the forward's own host
// code -- the same hs_plan, hsd_prepare, run_chain, pipe_takes_launch -- on placeholder addresses with a recorder installed on
// the calling thread, so a record cannot disagree with what a forward of that size launches.  Outside those calls the
// recorder is null and a launch function pays one thread-local load for it.
#pragma once
#include <stdint.h>

#include "../../include/adx.h"

namespace adx {

// kernel families (include/adx.h: ADX_PLAN_*)
enum PlanFamily {
  kPlanAux = ADX_PLAN_AUX,        // not a convolution: the time / condition embedding, the ticket reset, the attention block's LayerNorm and core
  kPlanPipe = ADX_PLAN_PIPE,       // tconv_pipe: the deepest level's seven convs
  kPlanChain = ADX_PLAN_CHAIN,      // tconv_chain: a whole level
  kPlanKsplit = ADX_PLAN_KSPLIT,     // tconv_hs_kernel
  kPlanShortK = ADX_PLAN_SHORTK,     // tconv_hsd_kernel
  kPlanShortKPair = ADX_PLAN_SHORTK_PAIR, // tconv_hsd_pair_kernel: two short-K convs
  kPlanMixed = ADX_PLAN_MIXED,      // tconv_hs_mixed_kernel: a K-split conv beside a short-K conv
  kPlanGeneric = ADX_PLAN_GENERIC,    // tconv_generic_kernel
  kPlanExact = ADX_PLAN_EXACT,      // tconv_kernel (exact fp32 MFMA)
  kPlanReduce = ADX_PLAN_REDUCE,     // tconv_hs_reduce_kernel behind a split launch that had no ticket words
};

struct PlanLaunch {
  int family = kPlanAux;
  int aux = 0;                     // kPlanAux: 1 embedding, 2 ticket reset, 3 attention LayerNorm, 4 attention core
  const void* w = nullptr;         // the (first) conv's weight image: names the layer
  const void* w_b = nullptr;       // pair / mixed: the second conv's
  int rows = 0, bt = 0;            // samples of the call, samples per row tile
  int ctiles = 0, ctiles_b = 0;    // workgroups along the channels (of the second conv of a pair / mixed launch)
  int grid = 0;
  int ksplit = 1;
  int reduce = 0;                  // ksplit > 1: 1 ticket words, 2 a reduce launch follows
  int chunks = 1;                  // staged input chunks a workgroup walks
  int vec_stage = 0, fast_epi = 0, ntap = 0;
  int ck = 0, cin_pad = 0;         // channels per staged chunk, padded input channels
  long long part_floats = 0;       // ksplit > 1: floats of partial tiles in the scratch
  const void* part = nullptr;      // ... and where they start
  long long lds_bytes = 0;
  int lout = 0, cout = 0;
};

struct PlanSink {
  PlanLaunch* rec = nullptr;
  int cap = 0, n = 0;
  bool assume_packed = false;      // plan as in a process whose device already holds the forward-number counter (adx_unet_pack made it)
};

PlanSink* plan_sink();             // the calling thread's recorder; null: launch
void plan_set_sink(PlanSink* s);
int plan_emit(PlanSink* s, const PlanLaunch& l);      // ADX_OK, or ADX_ERR_INVALID when the caller's array is full

// one launch as the ADX_PLAN_INTS words of include/adx.h; `layer` = {group, block, conv, block_b, conv_b}
void plan_write(const PlanLaunch& l, const int layer[5], long long part_off, int32_t* out);

// installs a recorder on the calling thread for the life of the scope
struct PlanScope {
  explicit PlanScope(PlanSink* s) { plan_set_sink(s); }
  ~PlanScope() { plan_set_sink(nullptr); }
};

}  // namespace adx
