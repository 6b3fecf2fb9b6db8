// omf_common.h — shared device/host helpers of the MI355X codec (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <string>

namespace omf {

constexpr int kThreads = 256;           // 4 wave64 per workgroup
constexpr int kWaves = kThreads / 64;

// Events that only order launches between streams of one device: no timing and no system-scope
// fence.  Recording an event with the default system-scope release writes back and invalidates
// the caches, and the next kernel on the stream started ~6 us later (rocprofv3 kernel trace, every
// encode call of round 3); the kernels' own completion already releases at device scope.
constexpr unsigned kOrderEventFlags = hipEventDisableTiming | hipEventDisableSystemFence;

// Top-K encoder counters of a plan (omf_topk_stats) that the host knows: calls of the sampled
// path and of the exact path.  Which path a sampled call took (bucket-sort fast path, zero fill,
// the exact tail's fallback, a redo) is decided on the device, which counts it (topk_exact_tail, omf_topk_exact.hip).
struct TopkStats {
  int64_t calls = 0, exact = 0;
};

// Top-K encoder settings of a plan (omf_topk.hip; its units' launchers use them): in experiment builds read from the
// OMF_TOPK_* environment once, at the plan's first Top-K call, and settable by the omf_plan_set_topk test hook.
struct TopkKnobs {
  TopkStats stats;
  bool init = false;
  int32_t groups = 1;          // two-stream group pipeline (off: measured slower)
  int32_t dbg = 0;             // OMF_TOPK_DBG diagnostics
  int32_t force_fallback = 0;  // 1: always the exact tail's radix sort; 2: and a barrier expiry (tests)
  int64_t sample_runs = 0;     // sampled runs per tensor at most (0: the default, 2 Ki)
  float sure_z = 1.5f, sure_c = 2.0f;  // the "sure" bin's margin below the expected rank-k count
  bool scatter_small = true;   // the bucket scatter's LDS-staged bucket table (OMF_TOPK_SCATTER_SMALL=0 off)
  bool planned_scatter = true; // the bucket plan inside the scatter launch (OMF_TOPK_PLANNED_SCATTER=0 off)
};

// Tuning knobs from the environment (OMF_TOPK_*, OMF_SPEC_*, OMF_RING_*, OMF_ENCODE_STRATEGY,
// OMF_DEC_LDS): read only by experiment builds (-DOMF_EXPERIMENTS, scripts/exp/variant_lib.sh);
// the product library ignores its environment and takes settings through the API alone
// (omf_codec_experimental.h for the test / experiment hooks).
inline const char* knob(const char* name) {
#ifdef OMF_EXPERIMENTS
  return std::getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}

// Thread-local error string behind omf_last_error().
void set_error(const std::string& msg);
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);

#define OMF_HIP(call)                                   \
  do {                                                  \
    hipError_t e_ = (call);                             \
    if (e_ != hipSuccess) return ::omf::hip_fail(e_, #call); \
  } while (0)

// Restores the caller's current device on scope exit.
struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// ---------------------------------------------------------------- device helpers

// One dword of every lane moved by a DPP control that reads no lane out of range (all rows and banks
// written; bound_ctrl set, so the destination needs no initial value).
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_mov(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ double dpp_mov_f64(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return __longlong_as_double((long long)(((uint64_t)dpp_mov<CTRL>((uint32_t)(b >> 32)) << 32) | dpp_mov<CTRL>((uint32_t)b)));
}

// Butterfly sum of a full wave, result in every lane: v += v[lane ^ o] for o = 32, 16, 8, 4, 2, 1 (the
// fp64 bits depend on this pairing tree; every strategy's norm is built on it).  No LDS traffic:
//   o = 32, 16  v_permlane32_swap / v_permlane16_swap of v with itself leave {own half | partner half}
//               in the two results, whose sum is v + v[lane ^ o] in both halves (+ commutes exactly);
//   o = 8       DPP row_ror:8;
//   o = 4       lane ^ 7 (DPP row_half_mirror) then lane ^ 3 (quad_perm [3,2,1,0]);
//   o = 2, 1    DPP quad_perm [2,3,0,1] / [1,0,3,2].
// Every lane of the wave must be active (each call site is wave-uniform).
__device__ __forceinline__ double wave_sum_f64(double v) {
  {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)b, hi = (uint32_t)(b >> 32);
    const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    v = __longlong_as_double((long long)(((uint64_t)h[0] << 32) | l[0])) +
        __longlong_as_double((long long)(((uint64_t)h[1] << 32) | l[1]));
  }
  {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)b, hi = (uint32_t)(b >> 32);
    const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    v = __longlong_as_double((long long)(((uint64_t)h[0] << 32) | l[0])) +
        __longlong_as_double((long long)(((uint64_t)h[1] << 32) | l[1]));
  }
  v += dpp_mov_f64<0x128>(v);                      // row_ror:8
  v += dpp_mov_f64<0x1B>(dpp_mov_f64<0x141>(v));   // row_half_mirror, then quad_perm [3,2,1,0]
  v += dpp_mov_f64<0x4E>(v);                       // quad_perm [2,3,0,1]
  v += dpp_mov_f64<0xB1>(v);                       // quad_perm [1,0,3,2]
  return v;
}

// Deterministic block sum (fixed butterfly per wave, fixed wave order); result valid in all threads.
__device__ __forceinline__ double block_sum_f64(double v, double* lds /* kWaves */) {
  v = wave_sum_f64(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  double s = lds[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) s += lds[w];
  __syncthreads();
  return s;
}

// Agent-scope relaxed accesses (global_load/store ... sc1): the hand-off protocol of
// cdna_hip_programming.md §6 G16 — payload stored sc1 + drained, consumer loads sc1.
__device__ __forceinline__ uint64_t ld_agent(const uint64_t* p) {
  return __hip_atomic_load(const_cast<uint64_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(uint64_t* p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t add_agent(uint32_t* p, uint32_t v) {
  return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void drain_vmem() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Philox4x32-10 (Salmon et al., SC'11).  Counter layout: oracle/philox.py.
// Each round's two 32x32->64 products are single 64-bit multiplies (v_mad_u64_u32).
#ifndef OMF_PHILOX_ROUNDS
#define OMF_PHILOX_ROUNDS 10
#endif
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < OMF_PHILOX_ROUNDS; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint64_t p0 = (uint64_t)0xD2511F53u * c.x;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c.z;
    // three-input xor in one v_bitop3_b32 (truth table 0x96)
    c = make_uint4(__builtin_amdgcn_bitop3_b32((uint32_t)(p1 >> 32), c.y, k0, 0x96), (uint32_t)p1,
                   __builtin_amdgcn_bitop3_b32((uint32_t)(p0 >> 32), c.w, k1, 0x96), (uint32_t)p0);
  }
  return c;
}

// 24-bit uniform in [0,1): the torch CPU generator's rule.
__device__ __forceinline__ float u24(uint32_t w) { return (float)(w & 0xFFFFFFu) * 5.9604644775390625e-08f; }

// Four 24-bit uniforms from three consecutive 32-bit words (96 bits, little-endian fields).
// The two fields that straddle a word are one byte permute each (v_perm_b32: selector bytes 0-3 take
// the second operand's bytes, 4-7 the first's, 0x0c is a zero byte): shift and mask in one instruction.
__device__ __forceinline__ float4 u24x4(uint32_t w0, uint32_t w1, uint32_t w2) {
  constexpr float k = 5.9604644775390625e-08f;
  return make_float4(u24(w0), (float)__builtin_amdgcn_perm(w1, w0, 0x0c050403u) * k,  // {w0.b3, w1.b0, w1.b1, 0}
                     (float)__builtin_amdgcn_perm(w2, w1, 0x0c040302u) * k,           // {w1.b2, w1.b3, w2.b0, 0}
                     (float)(w2 >> 8) * k);
}

// Correctly rounded x / d from r = RN(1/d): Markstein's theorem (one Newton step brings
// q within 1 ulp, the second fma-corrected step rounds correctly).  Valid for d in
// [2^-100, 2^100] and |x| >= 2^-96 or x == 0; callers take x / d elsewhere
// (scripts/exp/div_check.c: 0 mismatches in 1e9 random and near-halfway cases).
// A zero's quotient is a zero whose sign is not IEEE's: the correction steps add +0, so
// -0 / d with d > 0 gives +0.  A caller that stores the quotient fixes the sign itself.
__device__ __forceinline__ float div_markstein(float x, float d, float r) {
  float q = __fmul_rn(x, r);
  float e = fmaf(-q, d, x);
  q = fmaf(e, r, q);
  e = fmaf(-q, d, x);
  return fmaf(e, r, q);
}

__device__ __forceinline__ bool div_needs_exact(float x) {
  const float a = fabsf(x);
  return a != 0.0f && !(a >= 0x1p-96f);  // tiny non-zero (or NaN): exact division
}

typedef float f32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_nt(float* p, float4 v) {
  f32x4_t t = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(t, reinterpret_cast<f32x4_t*>(p));
}
__device__ __forceinline__ void store_nt(uint32_t* p, uint32_t v) { __builtin_nontemporal_store(v, p); }
typedef int i32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_nt(int32_t* p, int4 v) {
  i32x4_t t = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(t, reinterpret_cast<i32x4_t*>(p));
}

}  // namespace omf
