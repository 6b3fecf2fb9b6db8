// omf_topk_recv.hip — the receive side of Top-K, MI355X (gfx950): decode and checks of a selection.
//
// It consumes a message nobody here encoded: values and tensor-local int64 indices packed per tensor, in
// the layout of a ratio (k_t = omf_topk_k) or of the message's own per-tensor counts (k_t may be 0), with
// whatever indices the sender wrote — padding (-1), out of range, numpy-style negative, repeated.
// Decode modes: 0 zero-fill, 1 overlay (y[i] = v), 2 scatter-add (y[i] += v).  One tensor: topk_scatter;
// a whole client: topk_scatter_arena, or — mode 0 with a workspace — the tiled decode (topk_dec_place /
// topk_dec_tiles / topk_dec_overflow, one streaming write of the arena).  Before a decode,
// omf_topk_check_indices (topk_check_idx) and omf_topk_check_duplicates (topk_dup_bits<>).
// The tables and the workspace carve: omf_topk_layout.h (DecodeTables, DecTable, DecWs; CPU-tested).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/omf_codec.h"
#include "omf_common.h"
#include "omf_plan.h"
#include "omf_topk_dev.h"
#include "omf_topk_layout.h"

using namespace omf;
using namespace omf::topk_layout;  // the constants and tables shared with the host side

namespace {

__global__ __launch_bounds__(kThreads) void topk_scatter(const float* __restrict__ values,
                                                         const int64_t* __restrict__ indices, int64_t k,
                                                         float* __restrict__ y, int64_t n, int add) {
  for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < k; j += (int64_t)gridDim.x * kThreads) {
    const int64_t i = indices[j];
    if (i < 0 || i >= n) continue;
    y[i] = add ? __fadd_rn(y[i], values[j]) : values[j];
  }
}

// Whole-arena decode of one client's selection (values/indices packed per tensor at
// koff[t] = sum_{u<t} k_u, tensor-local indices): y[begin_t + idx] = v (mode 0/1) or += v (2).
// Indices are unique within a client, so the read-modify-write needs no atomics.  koff comes from
// the plan's decode table (a ratio's k_t, or a received message's counts; k_t may be 0).
__global__ __launch_bounds__(kThreads) void topk_scatter_arena(const float* __restrict__ values,
                                                               const int64_t* __restrict__ indices,
                                                               const int64_t* __restrict__ sizes,
                                                               const int64_t* __restrict__ begins,
                                                               const int64_t* __restrict__ koff_g, int nt,
                                                               int64_t ktot, float* __restrict__ y, int add) {
  __shared__ int64_t koff[kArenaMaxTensors + 1];
  for (int t = threadIdx.x; t <= nt; t += kThreads) koff[t] = koff_g[t];
  __syncthreads();
  for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < ktot; j += (int64_t)gridDim.x * kThreads) {
    const int t = koff_tensor(koff, 0, nt - 1, j);
    const int64_t i = indices[j];
    if (i < 0 || i >= sizes[t]) continue;  // padding (-1) or out of range: skipped
    float* p = y + begins[t] + i;
    *p = add ? __fadd_rn(*p, values[j]) : values[j];
  }
}

// Index check of a received selection, before anything is decoded: numpy's indexing of the
// reference decoder (`dense[indices] = values`, global_grpc_compression.py:154/158) wraps an index
// in [-n, 0) to i + n (rewritten here in place) and raises IndexError for one outside [-n, n).
// The lowest tensor holding such an index is atomicMin'ed into *bad (one atomic per wave).
__global__ __launch_bounds__(kThreads) void topk_check_idx(int64_t* __restrict__ indices,
                                                           const int64_t* __restrict__ sizes,
                                                           const int64_t* __restrict__ koff_g, int nt, int64_t ktot,
                                                           int32_t* __restrict__ bad) {
  __shared__ int64_t koff[kArenaMaxTensors + 1];
  for (int t = threadIdx.x; t <= nt; t += kThreads) koff[t] = koff_g[t];
  __syncthreads();
  int lowest = 0x7fffffff;
  for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < ktot; j += (int64_t)gridDim.x * kThreads) {
    const int t = koff_tensor(koff, 0, nt - 1, j);
    const int64_t i = indices[j], n = sizes[t];
    if (i >= n || i < -n) lowest = min(lowest, t);
    else if (i < 0) indices[j] = i + n;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lowest = min(lowest, __shfl_xor(lowest, o, 64));
  if ((threadIdx.x & 63) == 0 && lowest != 0x7fffffff) atomicMin(bad, lowest);
}

// Repeated indices of a received selection (omf_topk_check_duplicates): the reference decodes a
// layer as dense[indices] = values (numpy: the last value of a repeated index wins), which a
// scatter does not reproduce.  MARK sets each (in-range, wrapped) index's bit of an arena bitmap
// (plan-owned, all zero between calls) and flags the tensor whose bit was already set; the clear
// pass resets the bits it touched, so the bitmap is zero again for the next call.
template <bool MARK>
__global__ __launch_bounds__(kThreads) void topk_dup_bits(const int64_t* __restrict__ indices,
                                                          const int64_t* __restrict__ sizes,
                                                          const int64_t* __restrict__ tbegin,
                                                          const int64_t* __restrict__ koff_g, int nt, int64_t ktot,
                                                          uint32_t* __restrict__ bits, int32_t* __restrict__ flags) {
  __shared__ int64_t koff[kArenaMaxTensors + 1];
  for (int t = threadIdx.x; t <= nt; t += kThreads) koff[t] = koff_g[t];
  __syncthreads();
  for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < ktot; j += (int64_t)gridDim.x * kThreads) {
    const int t = koff_tensor(koff, 0, nt - 1, j);
    const int64_t i = indices[j];
    if (i < 0 || i >= sizes[t]) continue;  // out of range: omf_topk_check_indices reports it
    const uint64_t pos = (uint64_t)(tbegin[t] + i);
    const uint32_t b = 1u << (pos & 31);
    if (MARK) {
      if (atomicOr(&bits[pos >> 5], b) & b) flags[t] = 1;
    } else {
      atomicAnd(&bits[pos >> 5], ~b);
    }
  }
}

// ---------------------------------------------------------------- tiled zero-fill decode (mode 0)
// y := 0 over the whole arena, then y[begin_t + idx] = v for one client's selection, as ONE
// streaming write of the arena: the scattered 4-byte stores of a fill-then-scatter decode reach
// HBM as partial-line read-modify-writes (3.7x their bytes, profiles/r02).  So the values are
// first placed into per-super-tile buckets (64 Ki arena elements each; a bucket's capacity is
// twice the selection's expected count there + 256, fixed per (plan, ratio); what does not fit
// goes to an overflow list), then one workgroup per super-tile stages its bucket in LDS, builds
// each 16 Ki-element sub-tile in LDS (zeros + its values) and streams it out with 16-byte
// non-temporal stores; a last kernel applies the (normally empty) overflow list.
// The OMF_DEC_* macros are -D overrides for a variant library built with scripts/exp/variant_lib.sh.
#ifndef OMF_DEC_SUB_BITS
#define OMF_DEC_SUB_BITS 14
#endif
constexpr int kDecSubBits = OMF_DEC_SUB_BITS;
constexpr int kDecSubs = 1 << (kDecSuperBits - kDecSubBits);
#ifndef OMF_DEC_TILE_THREADS
#define OMF_DEC_TILE_THREADS 512
#endif
constexpr int kDecTileThreads = OMF_DEC_TILE_THREADS;
#ifndef OMF_DEC_STAGE
#define OMF_DEC_STAGE 2048
#endif
#ifndef OMF_DEC_MASK  // 1: a bit per tile element instead of a zeroed tile (measured, not faster)
#define OMF_DEC_MASK 0
#endif
constexpr int kDecStage = OMF_DEC_STAGE;  // bucket entries a tile workgroup stages in LDS (more: read from L2)

// Place one block of kDecChunk consecutive selected values into their super-tiles' buckets:
// LDS counts over the block's super-tile range, one global reservation per touched super-tile,
// then (position in the super-tile << 32 | value bits) at its slot, or into the overflow list
// (arena position << 32 | value bits) past the bucket's capacity.  The block's first and last
// tensor come from the plan's per-ratio table (blk_t); a block that spans several tensors (the
// small ones) finds each value's tensor by a binary search of their koff staged in LDS.
constexpr int kDecWin = 512;
__global__ __launch_bounds__(kThreads) void topk_dec_place(const float* __restrict__ values,
                                                           const int64_t* __restrict__ indices,
                                                           const int64_t* __restrict__ sizes,
                                                           const int64_t* __restrict__ begins,
                                                           const int64_t* __restrict__ koff,
                                                           const uint32_t* __restrict__ blk_t, int64_t ktot,
                                                           const uint32_t* __restrict__ cap_base,
                                                           uint32_t* __restrict__ fill, uint64_t* __restrict__ pairs,
                                                           uint32_t* __restrict__ ovf_cnt, uint64_t* __restrict__ ovf) {
  extern __shared__ uint32_t h[];  // the block's super-tile range (dynamic, <= kDecMaxSuper)
  __shared__ int64_t s_koff[kDecWin + 1];
  const int64_t j0 = (int64_t)blockIdx.x * kDecChunk, j1 = min(j0 + kDecChunk, ktot);
  const int tf = (int)blk_t[2 * blockIdx.x], tl = (int)blk_t[2 * blockIdx.x + 1];
  const bool win = tl - tf < kDecWin;
  if (tf != tl && win)
    for (int i = threadIdx.x; i <= tl - tf; i += kThreads) s_koff[i] = koff[tf + i];
  const uint32_t s_lo = (uint32_t)(begins[tf] >> kDecSuperBits);
  const uint32_t nbin = (uint32_t)((begins[tl] + sizes[tl] - 1) >> kDecSuperBits) - s_lo + 1;
  for (uint32_t b = threadIdx.x; b < nbin; b += kThreads) h[b] = 0;
  constexpr int U = kDecChunk / kThreads;
  int64_t pos[U];
  float val[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {  // every load issued before any is used
    const int64_t j = min(j0 + threadIdx.x + (int64_t)u * kThreads, j1 - 1);
    pos[u] = indices[j];
    val[u] = values[j];
  }
  __syncthreads();  // h zeroed
  uint32_t rank[U];
  if (tf == tl) {
    const int64_t n = sizes[tf], b0 = begins[tf];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = j0 + threadIdx.x + (int64_t)u * kThreads;
      const int64_t i = pos[u];
      pos[u] = (j >= j1 || i < 0 || i >= n) ? -1 : b0 + i;  // padding / out of range: skipped
      rank[u] = pos[u] >= 0 ? atomicAdd(&h[(uint32_t)(pos[u] >> kDecSuperBits) - s_lo], 1u) : 0u;
    }
  } else {
    int tt[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = min(j0 + threadIdx.x + (int64_t)u * kThreads, j1 - 1);
      if (win) {  // koff[t] <= j < koff[t + 1], in LDS
        int lo = 0, hi = tl - tf;
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (s_koff[mid] <= j) lo = mid;
          else hi = mid - 1;
        }
        tt[u] = tf + lo;
      } else {
        tt[u] = koff_tensor(koff, tf, tl, j);
      }
    }
    int64_t n[U], b0[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      n[u] = sizes[tt[u]];
      b0[u] = begins[tt[u]];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = j0 + threadIdx.x + (int64_t)u * kThreads;
      const int64_t i = pos[u];
      pos[u] = (j >= j1 || i < 0 || i >= n[u]) ? -1 : b0[u] + i;  // padding / out of range: skipped
      rank[u] = pos[u] >= 0 ? atomicAdd(&h[(uint32_t)(pos[u] >> kDecSuperBits) - s_lo], 1u) : 0u;
    }
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < nbin; b += kThreads)
    if (h[b]) h[b] = atomicAdd(&fill[s_lo + b], h[b]);  // this block's first slot in the bucket
  __syncthreads();
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (pos[u] < 0) continue;
    const uint32_t s = (uint32_t)(pos[u] >> kDecSuperBits);
    const uint32_t slot = h[s - s_lo] + rank[u], base = cap_base[s], cap = cap_base[s + 1] - base;
    const uint64_t vb = (uint64_t)__float_as_uint(val[u]);
    if (slot < cap) {
      pairs[(uint64_t)base + slot] = ((uint64_t)(pos[u] & ((1 << kDecSuperBits) - 1)) << 32) | vb;
    } else {  // bucket full (a selection far denser here than expected): the overflow list
      ovf[atomicAdd(ovf_cnt, 1u)] = ((uint64_t)pos[u] << 32) | vb;
    }
  }
}

// One workgroup per super-tile: its bucket staged in LDS (up to kDecStage entries; a larger
// one is read from L2 per sub-tile), then per 16 Ki-element sub-tile: zeros in LDS, its values,
// 16-byte non-temporal stores (the arena's partial last sub-tile element by element).
__global__ __launch_bounds__(kDecTileThreads) void topk_dec_tiles(const uint64_t* __restrict__ pairs,
                                                                  const uint32_t* __restrict__ cap_base,
                                                                  uint32_t* __restrict__ fill,
                                                                  float* __restrict__ y, int64_t arena_end) {
  __shared__ float4 tile[(1 << kDecSubBits) / 4];
  __shared__ uint64_t stage[kDecStage];
  __shared__ uint32_t s_fill;
#if OMF_DEC_MASK
  __shared__ uint32_t s_mask[(1 << kDecSubBits) / 32];  // which tile elements this sub-tile set
#endif
  float* tf = reinterpret_cast<float*>(tile);
  const uint32_t s = blockIdx.x;
  const uint32_t base = cap_base[s];
  if (threadIdx.x == 0) {  // read the bucket's count and leave it zero for the next call
    s_fill = fill[s];
    fill[s] = 0u;
  }
  __syncthreads();
  const uint32_t cnt = min(s_fill, cap_base[s + 1] - base);
  const bool staged = cnt <= (uint32_t)kDecStage;
  const uint64_t* src = staged ? stage : pairs + base;
  if (staged)
    for (uint32_t p = threadIdx.x; p < cnt; p += kDecTileThreads) stage[p] = pairs[base + p];
  constexpr int Q = (1 << kDecSubBits) / 4 / kDecTileThreads;  // float4 per thread per sub-tile
  for (int sub = 0; sub < kDecSubs; ++sub) {
    const int64_t b0 = ((int64_t)s << kDecSuperBits) + ((int64_t)sub << kDecSubBits);
    if (b0 >= arena_end) break;  // block-uniform
#if OMF_DEC_MASK
    // a bit per element instead of a zeroed tile: 2 KiB of LDS writes per sub-tile, not 64
    for (int i = threadIdx.x; i < (1 << kDecSubBits) / 32; i += kDecTileThreads) s_mask[i] = 0u;
    __syncthreads();  // (also: the staged bucket is complete)
    for (uint32_t p = threadIdx.x; p < cnt; p += kDecTileThreads) {
      const uint64_t pr = src[p];
      const uint32_t in = (uint32_t)(pr >> 32);
      if ((int)(in >> kDecSubBits) == sub) {
        const uint32_t l = in & ((1u << kDecSubBits) - 1);
        tf[l] = __uint_as_float((uint32_t)pr);
        atomicOr(&s_mask[l >> 5], 1u << (l & 31));
      }
    }
    __syncthreads();
    if (b0 + (1 << kDecSubBits) <= arena_end) {
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int e = 4 * (threadIdx.x + q * kDecTileThreads);
        const uint32_t m = (s_mask[e >> 5] >> (e & 31)) & 0xfu;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m) {  // elements of this sub-tile's earlier contents are stale: take the set ones only
          const float4 t = tile[threadIdx.x + q * kDecTileThreads];
          o.x = (m & 1u) ? t.x : 0.f; o.y = (m & 2u) ? t.y : 0.f;
          o.z = (m & 4u) ? t.z : 0.f; o.w = (m & 8u) ? t.w : 0.f;
        }
        store_nt(y + b0 + e, o);
      }
    } else {
      for (int64_t e = threadIdx.x; b0 + e < arena_end; e += kDecTileThreads)
        y[b0 + e] = ((s_mask[e >> 5] >> (e & 31)) & 1u) ? tf[e] : 0.f;
    }
    __syncthreads();
#else
#pragma unroll
    for (int q = 0; q < Q; ++q) tile[threadIdx.x + q * kDecTileThreads] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();  // (also: the staged bucket is complete)
    for (uint32_t p = threadIdx.x; p < cnt; p += kDecTileThreads) {
      const uint64_t pr = src[p];
      const uint32_t in = (uint32_t)(pr >> 32);
      if ((int)(in >> kDecSubBits) == sub) tf[in & ((1u << kDecSubBits) - 1)] = __uint_as_float((uint32_t)pr);
    }
    __syncthreads();
    if (b0 + (1 << kDecSubBits) <= arena_end) {
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int e = 4 * (threadIdx.x + q * kDecTileThreads);
        store_nt(y + b0 + e, tile[threadIdx.x + q * kDecTileThreads]);
      }
    } else {
      for (int64_t e = threadIdx.x; b0 + e < arena_end; e += kDecTileThreads) y[b0 + e] = tf[e];
    }
    __syncthreads();
#endif
  }
}

// The overflow list after the tiles (normally empty; one block), its count left zero for the next call.
__global__ __launch_bounds__(kThreads) void topk_dec_overflow(uint32_t* __restrict__ ovf_cnt,
                                                              const uint64_t* __restrict__ ovf, float* __restrict__ y) {
  const uint32_t n = *ovf_cnt;
  for (uint32_t j = threadIdx.x; j < n; j += kThreads) {
    const uint64_t pr = ovf[j];
    y[pr >> 32] = __uint_as_float((uint32_t)pr);
  }
  __syncthreads();  // every thread has read the count
  if (threadIdx.x == 0 && n) *ovf_cnt = 0u;
}

// ---------------------------------------------------------------- host side
// Whole-arena decode.  Plan-owned constant tables per selection layout (omf_plan.h topk_table, keyed
// by the ratio; topk_table_counts, keyed by a received message's per-tensor counts) and the caller
// workspace of the tiled zero-fill decode: topk_layout's DecodeTables / DecTable / DecWs.
struct DecTables {
  DecTable dev{};
  int32_t nsuper = 0;
  uint64_t cap_total = 0;
};

// k_t of every tensor at `ratio` (omf_topk_k) and their sum; false when some k_t > n_t.
bool ratio_counts(const omf_plan* plan, double ratio, std::vector<int64_t>& ks, int64_t* ktot) {
  const std::vector<int64_t>& sizes = plan->sizes;
  ks.resize(sizes.size());
  *ktot = 0;
  for (size_t t = 0; t < sizes.size(); ++t) {
    ks[t] = omf_topk_k(sizes[t], ratio);
    if (ks[t] > sizes[t]) return false;
    *ktot += ks[t];
  }
  return true;
}

}  // namespace

// Explicit counts: 0 <= counts[t] <= n_t (a received selection of more values than its tensor
// has elements would need duplicates; the caller decodes such a layer on its own).  Shared with
// omf_topk_pack.hip (declared in omf_plan.h).
int omf::topk_check_counts(const omf_plan* plan, const int64_t* counts, int64_t* ktot) {
  if (!counts) return fail(OMF_EINVAL, "counts is NULL");
  const std::vector<int64_t>& sizes = plan->sizes;
  int64_t s = 0;
  for (size_t t = 0; t < sizes.size(); ++t) {
    if (counts[t] < 0 || counts[t] > sizes[t])
      return fail(OMF_EINVAL, "counts[t] must be in [0, sizes[t]] (tensor " + std::to_string(t) + ")");
    s += counts[t];
  }
  *ktot = s;
  return OMF_OK;
}

namespace {

uint64_t ratio_key(double ratio) {
  uint64_t k;
  std::memcpy(&k, &ratio, 8);
  return k;
}

// The plan's tables for the layout ks (computed and uploaded on first use; the bucket total is
// kept in the table's host word).  ratio != NULL: keyed by the ratio, else by the counts.
int dec_tables(omf_plan* p, const int64_t* ks, int64_t ktot, const double* ratio, DecTables* out) {
  out->nsuper = dec_nsuper(p->arena_end);
  const Carve<DecTable> carve = dec_table_carve(p->nt, out->nsuper, dec_place_blocks(ktot));
  bool fresh = false;
  uint64_t* host = nullptr;
  void* d = ratio ? topk_table(p, ratio_key(*ratio), carve.bytes(), &fresh, &host)
                  : topk_table_counts(p, ks, carve.bytes(), &fresh, &host);
  if (!d) return fail(OMF_ENOMEM, "Top-K decode: table allocation failed");
  out->dev = carve.bind(d);
  if (fresh) {
    const DecodeTables h = dec_tables_host(p->sizes, p->offsets, p->arena_end, ks);
    OMF_HIP(hipMemcpy(out->dev.koff, h.koff.data(), 8 * h.koff.size(), hipMemcpyHostToDevice));
    OMF_HIP(hipMemcpy(out->dev.cap_base, h.cap_base.data(), 4 * h.cap_base.size(), hipMemcpyHostToDevice));
    OMF_HIP(hipMemcpy(out->dev.blk_t, h.blk_t.data(), 4 * h.blk_t.size(), hipMemcpyHostToDevice));
    *host = h.cap_base.back();
  }
  out->cap_total = *host;
  return OMF_OK;
}

size_t dec_ws_bytes(const omf_plan* plan, const int64_t* ks, int64_t ktot) {
  const DecodeTables h = dec_tables_host(plan->sizes, plan->offsets, plan->arena_end, ks);
  return dec_ws_layout(h.nsuper, h.cap_base.back(), ktot).bytes();
}

// One client's whole selection in the layout ks into the arena y (modes 0 / 1 / 2).
int decode_layout(omf_plan* plan, const int64_t* ks, int64_t ktot, const double* ratio, const float* values,
                         const int64_t* indices, float* y, int32_t mode, void* ws, size_t ws_bytes, void* stream) {
  if (mode < 0 || mode > 2) return fail(OMF_EINVAL, "Top-K arena decode: mode must be 0, 1 or 2");
  if ((ktot && (!values || !indices)) || !y) return fail(OMF_EINVAL, "Top-K arena decode: NULL buffer");
  const int32_t nt = plan->nt;
  if (nt > kArenaMaxTensors) return fail(OMF_EINVAL, "Top-K arena decode: too many tensors (decode per tensor)");
  DeviceGuard g(plan->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  hipStream_t st = (hipStream_t)stream;
  const int64_t ae = plan->arena_end;
  DecTables tb;
  if (int r = dec_tables(plan, ks, ktot, ratio, &tb)) return r;
  if (mode == 0 && ws && tb.nsuper <= kDecMaxSuper) {
    // one streaming write of the arena (larger arenas: fill + scatter below)
    const Carve<DecWs> d = dec_ws_layout(tb.nsuper, tb.cap_total, ktot);
    if (ws_bytes < d.bytes()) return fail(OMF_EINVAL, "Top-K arena decode: workspace too small");
    if (((uintptr_t)ws & 255) || ((uintptr_t)y & 15)) return fail(OMF_EINVAL, "Top-K arena decode: misaligned buffer");
    const DecWs w = d.bind(ws);
    uint32_t *fill = w.fill, *ovf_cnt = fill + tb.nsuper;
    uint64_t *pairs = w.pairs, *ovf = w.ovf;
    // fill[] and the overflow count start at zero (a zero-filled workspace) and every call leaves
    // them so: topk_dec_tiles clears its bucket's count, topk_dec_overflow the overflow count (a
    // memset here was two fill kernels, ~10 us per decode)
    if (ktot > 0) {
      const dim3 gb((unsigned)dec_place_blocks(ktot));
      hipLaunchKernelGGL(topk_dec_place, gb, dim3(kThreads), 4 * (size_t)tb.nsuper, st, values, indices,
                         plan->d_sizes, plan->d_begins, (const int64_t*)tb.dev.koff, (const uint32_t*)tb.dev.blk_t,
                         ktot, (const uint32_t*)tb.dev.cap_base, fill, pairs, ovf_cnt, ovf);
    }
    hipLaunchKernelGGL(topk_dec_tiles, dim3((unsigned)tb.nsuper), dim3(kDecTileThreads), 0, st, (const uint64_t*)pairs,
                       (const uint32_t*)tb.dev.cap_base, fill, y, ae);
    if (ktot > 0) hipLaunchKernelGGL(topk_dec_overflow, dim3(1), dim3(kThreads), 0, st, ovf_cnt, (const uint64_t*)ovf, y);
    OMF_HIP(hipGetLastError());
    return OMF_OK;
  }
  if (mode == 0) OMF_HIP(hipMemsetAsync(y, 0, 4 * (size_t)ae, st));
  if (ktot == 0) return OMF_OK;
  const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((ktot + kThreads - 1) / kThreads, 4096));
  hipLaunchKernelGGL(topk_scatter_arena, dim3(gx), dim3(kThreads), 0, st, values, indices,
                     plan->d_sizes, plan->d_begins, (const int64_t*)tb.dev.koff, (int)nt,
                     ktot, y, mode == 2 ? 1 : 0);
  OMF_HIP(hipGetLastError());
  return OMF_OK;
}

}  // namespace

extern "C" {

size_t omf_topk_decode_workspace_bytes(const omf_plan* plan, double ratio) {
  if (!plan || !(ratio == ratio)) return 0;
  std::vector<int64_t> ks;
  int64_t ktot = 0;
  if (!ratio_counts(plan, ratio, ks, &ktot)) return 0;
  return dec_ws_bytes(plan, ks.data(), ktot);
}

int omf_topk_decode_arena(omf_plan* plan, double ratio, const float* values, const int64_t* indices, float* y,
                          int32_t mode, void* stream) {
  return omf_topk_decode_arena_ws(plan, ratio, values, indices, y, mode, nullptr, 0, stream);
}

int omf_topk_decode_arena_ws(omf_plan* plan, double ratio, const float* values, const int64_t* indices, float* y,
                             int32_t mode, void* ws, size_t ws_bytes, void* stream) {
  if (!plan) return fail(OMF_EINVAL, "plan is NULL");
  if (!(ratio == ratio)) return fail(OMF_EINVAL, "ratio is NaN");
  std::vector<int64_t> ks;
  int64_t ktot = 0;
  if (!ratio_counts(plan, ratio, ks, &ktot))
    return fail(OMF_EINVAL, "selected index k out of range (k > numel): compress_ratio too large");
  return decode_layout(plan, ks.data(), ktot, &ratio, values, indices, y, mode, ws, ws_bytes, stream);
}

size_t omf_topk_decode_counts_workspace_bytes(const omf_plan* plan, const int64_t* counts) {
  if (!plan || !counts) return 0;
  int64_t ktot = 0;
  if (topk_check_counts(plan, counts, &ktot)) return 0;
  return dec_ws_bytes(plan, counts, ktot);
}

int omf_topk_decode_counts(omf_plan* plan, const int64_t* counts, const float* values, const int64_t* indices, float* y,
                           int32_t mode, void* ws, size_t ws_bytes, void* stream) {
  if (!plan) return fail(OMF_EINVAL, "plan is NULL");
  int64_t ktot = 0;
  if (int r = topk_check_counts(plan, counts, &ktot)) return r;
  return decode_layout(plan, counts, ktot, nullptr, values, indices, y, mode, ws, ws_bytes, stream);
}

int omf_topk_check_indices(omf_plan* plan, const int64_t* counts, int64_t* indices, int32_t* bad, void* stream) {
  if (!plan) return fail(OMF_EINVAL, "plan is NULL");
  if (!bad) return fail(OMF_EINVAL, "omf_topk_check_indices: bad is NULL");
  int64_t ktot = 0;
  if (int r = topk_check_counts(plan, counts, &ktot)) return r;
  if (ktot && !indices) return fail(OMF_EINVAL, "omf_topk_check_indices: indices is NULL");
  const int32_t nt = plan->nt;
  if (nt > kArenaMaxTensors) return fail(OMF_EINVAL, "omf_topk_check_indices: too many tensors");
  DeviceGuard g(plan->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  hipStream_t st = (hipStream_t)stream;
  DecTables tb;
  if (int r = dec_tables(plan, counts, ktot, nullptr, &tb)) return r;
  OMF_HIP(hipMemsetAsync(bad, 0x7f, 4, st));  // 0x7f7f7f7f: no tensor
  if (ktot == 0) return OMF_OK;
  const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((ktot + 4 * kThreads - 1) / (4 * kThreads), 2048));
  hipLaunchKernelGGL(topk_check_idx, dim3(gx), dim3(kThreads), 0, st, indices, plan->d_sizes,
                     (const int64_t*)tb.dev.koff, (int)nt, ktot, bad);
  OMF_HIP(hipGetLastError());
  return OMF_OK;
}

int omf_topk_check_duplicates(omf_plan* plan, const int64_t* counts, const int64_t* indices, int32_t* flags,
                              void* stream) {
  if (!plan) return fail(OMF_EINVAL, "plan is NULL");
  if (!flags) return fail(OMF_EINVAL, "omf_topk_check_duplicates: flags is NULL");
  int64_t ktot = 0;
  if (int r = topk_check_counts(plan, counts, &ktot)) return r;
  if (ktot && !indices) return fail(OMF_EINVAL, "omf_topk_check_duplicates: indices is NULL");
  const int32_t nt = plan->nt;
  if (nt > kArenaMaxTensors) return fail(OMF_EINVAL, "omf_topk_check_duplicates: too many tensors");
  DeviceGuard g(plan->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  hipStream_t st = (hipStream_t)stream;
  OMF_HIP(hipMemsetAsync(flags, 0, 4 * (size_t)nt, st));
  if (ktot == 0) return OMF_OK;
  DecTables tb;
  if (int r = dec_tables(plan, counts, ktot, nullptr, &tb)) return r;
  // the bitmap is the plan's: a call on another stream than the plan's previous stateful launch
  // is ordered after it (include/omf_codec.h), so two checks never mark and clear it at once
  if (int r = plan_enter(plan, st)) return r;
  constexpr uint64_t kDupTag = 0xD0B1E5B17A9E0000ull;
  const size_t words = (size_t)((plan->arena_end + 31) / 32);
  bool fresh = false;
  uint64_t* host = nullptr;
  uint32_t* bits = static_cast<uint32_t*>(topk_table(plan, kDupTag, 4 * words, &fresh, &host));
  if (!bits) return fail(OMF_ENOMEM, "omf_topk_check_duplicates: bitmap allocation failed");
  if (fresh) OMF_HIP(hipMemsetAsync(bits, 0, 4 * words, st));
  const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((ktot + kThreads - 1) / kThreads, 2048));
  hipLaunchKernelGGL(topk_dup_bits<true>, dim3(gx), dim3(kThreads), 0, st, indices, plan->d_sizes,
                     plan->d_begins, (const int64_t*)tb.dev.koff, (int)nt, ktot, bits, flags);
  hipLaunchKernelGGL(topk_dup_bits<false>, dim3(gx), dim3(kThreads), 0, st, indices, plan->d_sizes,
                     plan->d_begins, (const int64_t*)tb.dev.koff, (int)nt, ktot, bits, flags);
  OMF_HIP(hipGetLastError());
  return plan_leave(plan, st);
}

int omf_topk_decode(const float* values, const int64_t* indices, int64_t k, float* y, int64_t n, int32_t mode,
                    void* stream) {
  if (k < 0 || n < 0 || mode < 0 || mode > 2) return fail(OMF_EINVAL, "omf_topk_decode: bad arguments");
  if (n > 0 && !y) return fail(OMF_EINVAL, "omf_topk_decode: y is NULL");
  if (k > 0 && (!values || !indices)) return fail(OMF_EINVAL, "omf_topk_decode: values/indices NULL");
  hipStream_t st = (hipStream_t)stream;
  if (mode == 0 && n > 0) OMF_HIP(hipMemsetAsync(y, 0, (size_t)n * 4, st));
  if (k == 0) return OMF_OK;
  const unsigned g = (unsigned)std::min<int64_t>((k + kThreads - 1) / kThreads, 4096);
  hipLaunchKernelGGL(topk_scatter, dim3(g), dim3(kThreads), 0, st, values, indices, k, y, n, mode == 2 ? 1 : 0);
  OMF_HIP(hipGetLastError());
  return OMF_OK;
}

}  // extern "C"
