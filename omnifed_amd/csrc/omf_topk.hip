// omf_topk.hip — Top-K sparsification with error feedback, MI355X (gfx950).
// Semantics: src/omnifed/hybrid/compression/topk.py:10-47 + core.py:19-37 (reference):
//   t' = residual + alpha * x ; k = max(1, int(n * ratio)) ; the k largest |t'| ;
//   residual := t' - desparse(values, indices)  (= t' with the selected slots set to t'-t').
// alpha is the client weighting param * batch_samples (global_grpc.py:101-123), fused in;
// alpha = 1 leaves x's bits unchanged.
// Unit map (no kernel here): this file is the encoder's host side — the plan's knobs, the workspace layout
// and the per-ratio table upload, the C entry points; omf_topk_encode validates, binds both, counts the
// call and hands it (TopkCall, omf_topk_enc.h) to the launchers of
//   omf_topk_sampled.hip  plans of <= 256 tensors of <= 2^25 elements: sample, streaming pass, fine
//                         histogram, bucket plan, scatter and sort, in pipeline groups;
//   omf_topk_exact.hip    topk_exact_tail, always enqueued behind those (the zero fill, the device-decided
//                         fallback), and the exact path of larger plans.
// The integer code (constants and per-tensor rules shared with the kernels, the constant tables, the pipeline
// groups, the workspace carve) is omf_topk_layout.{h,cpp}: no HIP header, CPU-tested; the plan: omf_plan.h.
// Decode and checks of a received selection: omf_topk_recv.hip.  The torch-order rewrite of a finished selection:
// omf_topk_tie.hip, which gets this unit's workspace carve and tables by omf::topk_encode_tables.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../../include/omf_codec.h"
#include "../../include/omf_codec_experimental.h"
#include "omf_common.h"
#include "omf_plan.h"
#include "omf_topk_enc.h"
#include "omf_topk_layout.h"

using namespace omf;
using namespace omf::topk_layout;  // the constants and per-tensor rules shared with the host side

namespace {

// The plan's Top-K settings: in experiment builds (omf::knob) the OMF_TOPK_* environment read once, at its first
// Top-K call (OMF_TOPK_GROUPS, OMF_TOPK_DBG, OMF_TOPK_FALLBACK, OMF_TOPK_SAMPLE_RUNS, OMF_TOPK_SURE="z,c",
// OMF_TOPK_SCATTER_SMALL, OMF_TOPK_PLANNED_SCATTER), unless omf_plan_set_topk set them first.
const TopkKnobs& knobs(omf_plan* p) {
  TopkKnobs& k = p->topk_knobs;
  if (k.init) return k;
  k.init = true;
  if (const char* e = omf::knob("OMF_TOPK_GROUPS")) k.groups = std::max(1, std::atoi(e));
  if (const char* e = omf::knob("OMF_TOPK_DBG")) {
    // 4 = print the verdict flags, 8 = print over-full fine bins; experiment builds only
    // (-DOMF_EXPERIMENTS; they change what an encode writes): 1 = no bucket sort, 2 = no residual zeroing
    const int d = std::atoi(e);
#ifdef OMF_EXPERIMENTS
    k.dbg = d;
#else
    k.dbg = d & ~3;
#endif
  }
  if (const char* e = omf::knob("OMF_TOPK_FALLBACK")) k.force_fallback = e[0] == '1';
  if (const char* e = omf::knob("OMF_TOPK_SCATTER_SMALL")) k.scatter_small = e[0] != '0';
  if (const char* e = omf::knob("OMF_TOPK_PLANNED_SCATTER")) k.planned_scatter = e[0] != '0';
  if (const char* e = omf::knob("OMF_TOPK_SAMPLE_RUNS")) {
    const long long v = std::atoll(e);
    if (v >= 64 && v <= (1 << 20)) k.sample_runs = v;
  }
  if (const char* e = omf::knob("OMF_TOPK_SURE")) {
    float z = 0.f, c = 0.f;
    if (std::sscanf(e, "%f,%f", &z, &c) == 2 && z >= 0.f && c >= 0.f) {
      k.sure_z = z;
      k.sure_c = c;
    }
  }
  return k;
}

bool global_path(const omf_plan* p) {
  if (p->nt > 256) return false;
  for (int64_t n : p->sizes)
    if (n > (int64_t)1 << 25) return false;
  return true;
}

// The caller workspace's layout (topk_layout::encode_ws_layout), kept in the plan: made at the plan's
// first Top-K use (sizing the library sort is not free, and every call needs it).
const EncodeWsLayout& encode_ws(const omf_plan* p) {
  std::call_once(p->topk_ws_once, [p] {
    p->topk_ws = encode_ws_layout(p->sizes, p->arena_end, topk_sort_tmp_bytes(p, global_path(p)));
  });
  return p->topk_ws;
}

// Runs sampled per tensor at most (a performance knob only: the selection is exact for any
// sample; TopkKnobs::sample_runs overrides it for experiments).
int64_t sample_max_runs(const TopkKnobs& kn) { return kn.sample_runs ? kn.sample_runs : (int64_t)kSMaxRuns; }

// The "sure" bin's margin below the expected rank-k sample count m: m - z sqrt(m) - c (a
// performance knob only: any sure bin gives the same selection — a sure key that is not selected
// after all gets its t' back).  Every selected key below the sure bin costs the bucket sort a
// random 4-byte residual store, every sure key past rank k one more: Llama-400M bucket sort 92 us
// at (6, 32), 67 at (1.5, 2), 66 at (1, 0) (round 3, rocprofv3).  TopkKnobs::sure_z / sure_c.
float2 sure_margin(const TopkKnobs& kn) { return make_float2(kn.sure_z, kn.sure_c); }

constexpr uint64_t kSetupTag = 0x5E7A9B1C00000000ull;
constexpr uint64_t kStatsTag = 0x57A7500D0000000Full;

// The plan's counters of the sampled path that the device decides (the exact tail updates them):
// [0] fast path, [1] zero fills, [2] fallbacks, [3] redos.  A plan-owned table, zeroed on creation.
unsigned long long* device_stats(omf_plan* p, hipStream_t st) {
  bool fresh = false;
  uint64_t* host = nullptr;
  void* d = topk_table(p, kStatsTag, 64, &fresh, &host);
  if (!d) return nullptr;
  if (fresh && hipMemsetAsync(d, 0, 64, st) != hipSuccess) return nullptr;
  return static_cast<unsigned long long*>(d);
}

// The encoder's constant tables for (ratio, sample size): topk_layout::build_encode_tables' vectors in a
// plan-owned device table (topk_table, omf_plan.h), uploaded once; the plan keeps the latest host and
// device side (EncodeSetup).  The call that makes a table also clears the workspace's four verdict
// words (the kernel that once computed these tables on the device wrote them too).
int setup_table(omf_plan* p, double ratio, int64_t max_runs, hipStream_t st, uint32_t* status,
                const EncodeSetup** out) {
  EncodeSetup& es = p->topk_setup;
  *out = &es;
  uint64_t bits;
  std::memcpy(&bits, &ratio, 8);
  if (es.valid && es.ratio_bits == bits && es.max_runs == max_runs) return OMF_OK;
  es.valid = false;
  es.host = build_encode_tables(p->sizes, ratio, max_runs);
  const EncodeTables& h = es.host;
  const SetupCarve sc = setup_table_carve(h);
  bool fresh = false;
  uint64_t* host = nullptr;
  const uint64_t key = bits ^ kSetupTag ^ ((uint64_t)max_runs * 0x9E3779B97F4A7C15ull);
  uint8_t* d = static_cast<uint8_t*>(topk_table(p, key, sc.carve.bytes(), &fresh, &host));
  if (!d) return fail(OMF_ENOMEM, "omf_topk_encode: table allocation failed");
  const SetupTable tb = sc.carve.bind(d);
  if (fresh) {
    OMF_HIP(hipMemsetAsync(tb.done, 0, sc.carve.bytes() - sc.zero_begin, st));  // the arrival counters, gz and gh
    OMF_HIP(hipMemsetAsync(status, 0, 16, st));
    auto up = [st](auto* dst, const auto& v) {
      return v.empty() ? hipSuccess : hipMemcpyAsync(dst, v.data(), sizeof(v[0]) * v.size(), hipMemcpyHostToDevice, st);
    };
    OMF_HIP(up(tb.kk, h.kk));
    OMF_HIP(up(tb.koff, h.koff));
    OMF_HIP(up(tb.kb2, h.kb2));
    OMF_HIP(up(tb.tfirst, h.tfirst));
    OMF_HIP(up(tb.tlast, h.tlast));
    OMF_HIP(up(tb.bbase, h.bbase));
    OMF_HIP(up(tb.sbase, h.sbase));
    OMF_HIP(up(tb.smap, h.smap));
    OMF_HIP(up(tb.supinfo, h.supinfo));
    OMF_HIP(up(tb.zmap, h.zmap));
    OMF_HIP(hipStreamSynchronize(st));  // once per (plan, ratio, sample size)
  }
  es.dev = tb;
  es.ratio_bits = bits;
  es.max_runs = max_runs;
  es.valid = true;
  return OMF_OK;
}

}  // namespace

int omf::topk_encode_tables(omf_plan* plan, double ratio, void* ws, size_t ws_bytes, hipStream_t st, EncodeWs* w,
                            SetupTable* tb) {  // omf_topk_enc.h
  const EncodeWsLayout& L = encode_ws(plan);
  if (ws_bytes < L.total) return fail(OMF_EINVAL, "workspace too small (see omf_topk_workspace_bytes)");
  DeviceGuard g(plan->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  *w = L.carve.bind(ws);
  const EncodeSetup* es = nullptr;
  if (int r = setup_table(plan, ratio, sample_max_runs(knobs(plan)), st, w->status, &es)) return r;
  *tb = es->dev;
  return OMF_OK;
}

extern "C" {

int64_t omf_topk_k(int64_t numel, double ratio) { return topk_k(numel, ratio); }

int omf_plan_set_topk(omf_plan* plan, int32_t groups, int32_t force_fallback, int64_t sample_runs, float sure_z,
                      float sure_c) {
  if (!plan) return fail(OMF_EINVAL, "plan is NULL");
  if (sample_runs > 0 && (sample_runs < 64 || sample_runs > (1 << 20)))
    return fail(OMF_EINVAL, "omf_plan_set_topk: sample_runs must be 0 (default) or in [64, 2^20]");
  (void)knobs(plan);  // the environment's values first, so a negative argument keeps them
  TopkKnobs& k = plan->topk_knobs;
  if (groups >= 1) k.groups = groups;
  if (force_fallback > 2) return fail(OMF_EINVAL, "omf_plan_set_topk: force_fallback must be 0, 1 or 2");
  if (force_fallback >= 0) k.force_fallback = force_fallback;
  if (sample_runs >= 0) k.sample_runs = sample_runs;
  if (sure_z >= 0.f) k.sure_z = sure_z;
  if (sure_c >= 0.f) k.sure_c = sure_c;
  return OMF_OK;
}

int omf_topk_stats(omf_plan* plan, int64_t* out6, int32_t reset) {
  if (!plan || !out6) return fail(OMF_EINVAL, "plan and out6 must be non-NULL");
  TopkStats& s = plan->topk_knobs.stats;
  DeviceGuard g(plan->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  OMF_HIP(hipDeviceSynchronize());  // the device keeps the path counters (the exact tail's)
  bool fresh = false;
  uint64_t* host = nullptr;
  void* d = topk_table(plan, kStatsTag, 64, &fresh, &host);
  if (!d) return fail(OMF_ENOMEM, "omf_topk_stats: counter table allocation failed");
  unsigned long long dv[4] = {0, 0, 0, 0};
  if (fresh) OMF_HIP(hipMemset(d, 0, 64));
  else OMF_HIP(hipMemcpy(dv, d, sizeof dv, hipMemcpyDeviceToHost));
  const int64_t v[6] = {s.calls, (int64_t)dv[0], (int64_t)dv[1], (int64_t)dv[2], (int64_t)dv[3], s.exact};
  std::memcpy(out6, v, sizeof v);
  if (reset) {
    s.calls = s.exact = 0;
    OMF_HIP(hipMemset(d, 0, sizeof dv));
  }
  return OMF_OK;
}

size_t omf_topk_workspace_bytes(const omf_plan* plan, double ratio) {
  (void)ratio;
  if (!plan) return 0;
  return encode_ws(plan).total;
}

int omf_topk_encode(omf_plan* plan, const float* x, float* residual, int32_t residual_mode, double ratio, float alpha,
                    float* values, int64_t* indices, void* ws, size_t ws_bytes, void* stream) {
  if (!plan) return fail(OMF_EINVAL, "plan is NULL");
  if (!x || !values || !indices || !ws) return fail(OMF_EINVAL, "x, values, indices and ws must be non-NULL");
  if (residual_mode < 0 || residual_mode > 2 || (residual_mode != 0 && !residual))
    return fail(OMF_EINVAL, "residual_mode must be 0 (none), 1 (compensate+update) or 2 (init) with a residual buffer");
  if (!(ratio == ratio)) return fail(OMF_EINVAL, "ratio is NaN");
  const std::vector<int64_t>& sizes = plan->sizes;
  int64_t kmax = 0;
  for (int64_t n : sizes) {
    const int64_t k = omf_topk_k(n, ratio);
    if (k > n) return fail(OMF_EINVAL, "selected index k out of range (k > numel): compress_ratio too large");
    if (n > 0x7fffffffLL) return fail(OMF_EINVAL, "tensor too large for 32-bit candidate indices");
    kmax = std::max(kmax, k);
  }
  if (plan->arena_end > 0xffffffffLL) return fail(OMF_EINVAL, "arena too large for the sort");
  if (((uintptr_t)x & 15) || (residual && ((uintptr_t)residual & 15)))
    return fail(OMF_EINVAL, "x and residual must be 16-byte aligned");
  const EncodeWsLayout& L = encode_ws(plan);
  if (ws_bytes < L.total) return fail(OMF_EINVAL, "workspace too small (see omf_topk_workspace_bytes)");
  DeviceGuard g(plan->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  hipStream_t st = (hipStream_t)stream;
  const bool glob = global_path(plan);
  if (!glob) OMF_HIP(hipMemsetAsync(ws, 0, L.zero_end, st));
  // the per-(plan, ratio) constant tables: built and uploaded on the first call at this ratio
  const EncodeSetup* es = nullptr;
  const TopkKnobs& kn = knobs(plan);
  const int64_t max_runs = sample_max_runs(kn);
  TopkCall c{.plan = plan, .x = x, .tp = residual_mode == 0 ? x : residual, .residual = residual,
             .rz = residual_mode ? residual : nullptr, .mode = residual_mode, .alpha = alpha,
             .scale = residual_mode == 0 ? alpha : 1.0f, .values = values, .indices = indices, .st = st,
             .w = L.carve.bind(ws), .tb = {}, .host = nullptr};
  if (int r = setup_table(plan, ratio, max_runs, st, c.w.status, &es)) return r;
  c.tb = es->dev;
  c.host = &es->host;
  if (!glob) {
    ++plan->topk_knobs.stats.exact;
    return topk_launch_exact(c, kmax, L.tmp_bytes);
  }
  unsigned long long* dstats = device_stats(plan, st);
  if (!dstats) return fail(OMF_ENOMEM, "omf_topk_encode: counter table allocation failed");
  if (int r = topk_launch_sampled(c, max_runs, sure_margin(kn))) return r;
  ++plan->topk_knobs.stats.calls;
  return topk_launch_tail(c, dstats);
}

}  // extern "C"
