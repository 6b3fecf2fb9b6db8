// omf_topk_enc.h — what the Top-K encoder (omf_topk.hip) gives the torch-order rewrite (omf_topk_tie.hip).
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
}  // namespace omf
