// omf_h16.h — internal interface of the 16-bit-arena QSGD encoder (omf_qsgd_h16.hip).
//
// Not part of the C ABI: omf_qsgd_encode_h16 / omf_qsgd_norms_h16 (omf_qsgd.hip) validate a call and hand
// it to omf::h16::launch.  DESIGN.md §3.5 describes the layout and the load shape.
#pragma once

#include "omf_bracket.h"  // EncCall, enc_args, launch_kernel

namespace omf {
namespace h16 {

// The sum-of-squares launch (skipped with caller norms) and the quantise launch (skipped for a norms-only
// call) of one encode of the bf16 / fp16 arena x16 on c.st; c.x is unused.  0 or an OMF_E* code.
__attribute__((visibility("hidden"))) int launch(omf_plan* p, const EncCall& c, const void* x16);

}  // namespace h16
}  // namespace omf
