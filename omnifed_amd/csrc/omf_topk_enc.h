// omf_topk_enc.h — the host-side seams of the Top-K encoder: what omf_topk.hip (validation, workspace, tables)
// gives its kernel units' launchers (omf_topk_sampled.hip, omf_topk_exact.hip) and omf_topk_tie.hip.
#pragma once
#include "omf_common.h"
#include "omf_plan.h"
#include "omf_topk_layout.h"

namespace omf {
// The encoder's view of a call at `ratio`: checks ws_bytes ("workspace too small", OMF_EINVAL), then on the
// plan's device binds the workspace's regions into *w and the per-(plan, ratio) tables — built and uploaded
// on `st` at the ratio's first use — into *tb.  OMF_OK or the failed step's error.
int topk_encode_tables(omf_plan* plan, double ratio, void* ws, size_t ws_bytes, hipStream_t st,
                       topk_layout::EncodeWs* w, topk_layout::SetupTable* tb);

// One omf_topk_encode call's operands: validated, on the plan's device, the plan's knobs (plan->topk_knobs)
// read.  Host only, never a kernel argument.
struct TopkCall {
  omf_plan* plan;
  const float *x, *tp;   // t' lives in the residual (EF modes) or is scale * x (mode 0)
  float *residual, *rz;  // rz: the residual for fix-ups (restores / zeroing), null in mode 0
  int32_t mode;          // residual_mode: 0 none, 1 compensate + update, 2 init
  float alpha, scale;    // scale: alpha in mode 0, else 1
  float* values;
  int64_t* indices;
  hipStream_t st;
  topk_layout::EncodeWs w;                // the caller's workspace, bound
  topk_layout::SetupTable tb;             // the (plan, ratio, sample size) tables on the device
  const topk_layout::EncodeTables* host;  // and their host side
};
// omf_topk_sampled.hip: the sampled path's pipeline groups, group 0 on c.st (joined there if there are more).
int topk_launch_sampled(const TopkCall& c, int64_t max_runs, float2 sure_zc);
// omf_topk_exact.hip: the exact tail behind those groups (dstats: the plan's path counters); the exact path of other
// plans (kmax: the largest k_t, tmp_bytes of c.w.tmp); those bytes (sampled: the exact tail's digit table instead).
int topk_launch_tail(const TopkCall& c, unsigned long long* dstats);
int topk_launch_exact(const TopkCall& c, int64_t kmax, size_t tmp_bytes);
size_t topk_sort_tmp_bytes(const omf_plan* p, bool sampled);
}  // namespace omf
