// omf_topk_pack.hip — the opt-in bit-packed Top-K index wire ("TopKBitPackedCompression"), MI355X (gfx950).
//
// NOT reference-compatible: a new compression_type a sender uses only when asked to.  The k tensor-local
// int64 indices of a tensor of n elements (global_grpc_compression.py:88-98 sends them as 8 bytes each)
// become b = index_bits(n) bits each, LSB-first little-endian, in the selection's order.  In a plan's
// packed arena a group of 32 consecutive indices of one tensor is exactly b words and starts on a word
// (tensor t's first group goff[t], first word woff[t]: omf_topk_layout.h PackTables, CPU-tested), so one
// thread packs or unpacks a group alone with the routines the host check runs (pack_group / unpack_group).
// The kernels move at most 12 bytes per selected element; they exist so that the int64 indices never
// cross PCIe.
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/omf_codec.h"
#include "omf_common.h"
#include "omf_plan.h"
#include "omf_qsgd_dec.h"  // aligned, overlaps
#include "omf_topk_dev.h"
#include "omf_topk_layout.h"

using namespace omf;
using namespace omf::topk_layout;

// The plan's device tables of the packed arena for `counts` (uploaded on first use; the last 8 count
// vectors kept) and the host facts a call needs.  Shared with omf_topk_qval.hip (declared in omf_plan.h).
int omf::topk_pack_args(omf_plan* plan, const int64_t* counts, PackArgs* out) {
  if (!plan) return fail(OMF_EINVAL, "plan is NULL");
  if (int r = topk_check_counts(plan, counts, &out->ktot)) return r;
  const PackTables h = pack_tables_host(plan->sizes, counts);
  if (h.words < 0) return fail(OMF_EINVAL, "the packed Top-K wire takes tensors of at most 2^32 elements");
  out->groups = h.goff.back();
  out->words = h.words;
  if (out->groups >= ((int64_t)1 << 32)) return fail(OMF_EINVAL, "the packed Top-K wire: too many indices");
  if (out->ktot == 0) return OMF_OK;  // nothing to launch: no table either
  DeviceGuard g(plan->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  const Carve<PackTable> carve = pack_table_carve(plan->nt);
  bool fresh = false;
  uint64_t* host = nullptr;
  void* d = topk_table_counts(plan, counts, carve.bytes(), &fresh, &host, kPackCountsKey);
  if (!d) return fail(OMF_ENOMEM, "packed Top-K wire: table allocation failed");
  out->dev = carve.bind(d);
  if (fresh) {
    const std::vector<uint32_t> goff32(h.goff.begin(), h.goff.end());
    OMF_HIP(hipMemcpy(out->dev.koff, h.koff.data(), 8 * h.koff.size(), hipMemcpyHostToDevice));
    OMF_HIP(hipMemcpy(out->dev.woff, h.woff.data(), 8 * h.woff.size(), hipMemcpyHostToDevice));
    OMF_HIP(hipMemcpy(out->dev.goff, goff32.data(), 4 * goff32.size(), hipMemcpyHostToDevice));
    OMF_HIP(hipMemcpy(out->dev.bits, h.bits.data(), 4 * h.bits.size(), hipMemcpyHostToDevice));
  }
  return OMF_OK;
}

namespace {

// One thread per group: its (at most 32) int64 indices read directly, as qsgd_pack reads its levels, and
// packed into b whole words — the code of an index is its low b bits, the codes after the tensor's k_t-th
// index are 0.
__global__ __launch_bounds__(kThreads) void topk_pack_idx(const int64_t* __restrict__ indices,
                                                          const int64_t* __restrict__ koff,
                                                          const int64_t* __restrict__ woff,
                                                          const uint32_t* __restrict__ goff,
                                                          const int32_t* __restrict__ bits, int nt, int64_t groups,
                                                          uint32_t* __restrict__ packed) {
  __shared__ uint32_t s_goff[kArenaMaxTensors + 1];
  stage_goff(goff, s_goff, nt);
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= groups) return;
  const int t = group_tensor(goff, s_goff, nt, g);
  const int64_t j = g - (int64_t)goff[t], k0 = koff[t];
  const int nv = (int)min((int64_t)kPackGroup, koff[t + 1] - k0 - kPackGroup * j);
  const int b = bits[t];
  const int64_t* src = indices + k0 + kPackGroup * j;
  int64_t v[kPackGroup];
#pragma unroll
  for (int i = 0; i < kPackGroup; ++i) v[i] = i < nv ? src[i] : 0;  // every load issued before a word is stored
  pack_group(v, nv, b, packed + woff[t] + j * b);
}

// One thread per group unpacks the group's first nv codes (reading only the words that hold them); the
// workgroup's indices — one contiguous run of at most 32 kThreads of the output — go through an LDS tile
// (position p at word p + p / 32: qsgd_decode_packed's 33-word rows when the groups are whole), so the
// int64 stores are lane-contiguous 16-byte stores of two indices each.  Positions count from the even
// element at or below the run's first, so that every pair is 16-byte aligned; a pair half outside the run
// is one 8-byte store.  Nothing past a tensor's k_t-th index is written.
constexpr int kTileWords = (kPackGroup + 1) * kThreads + 8;
__global__ __launch_bounds__(kThreads) void topk_unpack_idx(const uint32_t* __restrict__ packed,
                                                            const int64_t* __restrict__ koff,
                                                            const int64_t* __restrict__ woff,
                                                            const uint32_t* __restrict__ goff,
                                                            const int32_t* __restrict__ bits, int nt, int64_t groups,
                                                            int64_t* __restrict__ indices) {
  __shared__ uint32_t s_goff[kArenaMaxTensors + 1];
  __shared__ uint32_t tile[kTileWords];
  __shared__ int64_t s_run[2];  // the workgroup's run of the output: [first, end)
  stage_goff(goff, s_goff, nt);
  const int64_t g0 = (int64_t)blockIdx.x * kThreads, g = g0 + threadIdx.x;
  const bool live = g < groups;
  uint32_t c[kPackGroup] = {};
  int nv = 0;
  int64_t o0 = 0;
  if (live) {
    const int t = group_tensor(goff, s_goff, nt, g);
    const int64_t j = g - (int64_t)goff[t], k0 = koff[t];
    nv = (int)min((int64_t)kPackGroup, koff[t + 1] - k0 - kPackGroup * j);
    const int b = bits[t];
    o0 = k0 + kPackGroup * j;
    unpack_group(packed + woff[t] + j * b, nv, b, c);
    if (threadIdx.x == 0) s_run[0] = o0;
    if (g == min(groups, g0 + kThreads) - 1) s_run[1] = o0 + nv;
  }
  __syncthreads();
  const int64_t first = s_run[0];
  const int odd = (int)((((uintptr_t)indices >> 3) + (uint64_t)first) & 1);
  const int64_t base = first - odd;  // indices + base is 16-byte aligned
  const int end = odd + (int)(s_run[1] - first);  // the run's positions: [odd, end), end <= 32 kThreads + 1
  if (live) {
    const int p0 = (int)(o0 - base);
#pragma unroll
    for (int i = 0; i < kPackGroup; ++i)
      if (i < nv) tile[(p0 + i) + ((p0 + i) >> 5)] = c[i];
  }
  __syncthreads();
  for (int p = 2 * (int)threadIdx.x; p < end; p += 2 * kThreads) {
    const bool h0 = p >= odd, h1 = p + 1 < end;
    const uint64_t c0 = tile[p + (p >> 5)], c1 = tile[(p + 1) + ((p + 1) >> 5)];
    int64_t* o = indices + base + p;
    if (h0 && h1) *reinterpret_cast<ulonglong2*>(o) = make_ulonglong2(c0, c1);
    else if (h0) o[0] = (int64_t)c0;
    else if (h1) o[1] = (int64_t)c1;
  }
}

// The pointer rules of both calls: non-NULL, packed 4-byte and indices 8-byte aligned, disjoint.
int check_buffers(const PackArgs& a, const void* indices, const void* packed) {
  if (!indices || !packed) return fail(OMF_EINVAL, "indices and packed must be non-NULL");
  if (!aligned(packed, 4) || !aligned(indices, 8))
    return fail(OMF_EINVAL, "packed must be 4-byte, indices 8-byte aligned");
  if (overlaps(indices, 8 * (size_t)a.ktot, packed, 4 * (size_t)a.words))
    return fail(OMF_EINVAL, "indices and packed overlap");
  return OMF_OK;
}

}  // namespace

extern "C" {

int32_t omf_topk_index_bits(int64_t n) { return index_bits(n); }

int64_t omf_topk_packed_words(omf_plan* plan, const int64_t* counts) {
  int64_t ktot = 0;
  if (!plan || topk_check_counts(plan, counts, &ktot)) return -1;
  return pack_tables_host(plan->sizes, counts).words;
}

int omf_topk_pack_indices(omf_plan* plan, const int64_t* counts, const int64_t* indices, uint32_t* packed,
                          void* stream) {
  PackArgs a;
  if (int r = topk_pack_args(plan, counts, &a)) return r;
  if (a.ktot == 0) return OMF_OK;
  if (int r = check_buffers(a, indices, packed)) return r;
  DeviceGuard g(plan->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  const dim3 grid((unsigned)((a.groups + kThreads - 1) / kThreads));
  hipLaunchKernelGGL(topk_pack_idx, grid, dim3(kThreads), 0, (hipStream_t)stream, indices,
                     (const int64_t*)a.dev.koff, (const int64_t*)a.dev.woff, (const uint32_t*)a.dev.goff,
                     (const int32_t*)a.dev.bits, (int)plan->nt, a.groups, packed);
  OMF_HIP(hipGetLastError());
  return OMF_OK;
}

int omf_topk_unpack_indices(omf_plan* plan, const int64_t* counts, const uint32_t* packed, int64_t* indices,
                            void* stream) {
  PackArgs a;
  if (int r = topk_pack_args(plan, counts, &a)) return r;
  if (a.ktot == 0) return OMF_OK;
  if (int r = check_buffers(a, indices, packed)) return r;
  DeviceGuard g(plan->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  const dim3 grid((unsigned)((a.groups + kThreads - 1) / kThreads));
  hipLaunchKernelGGL(topk_unpack_idx, grid, dim3(kThreads), 0, (hipStream_t)stream, packed,
                     (const int64_t*)a.dev.koff, (const int64_t*)a.dev.woff, (const uint32_t*)a.dev.goff,
                     (const int32_t*)a.dev.bits, (int)plan->nt, a.groups, indices);
  OMF_HIP(hipGetLastError());
  return OMF_OK;
}

}  // extern "C"
