// omf_runtime.cpp — error reporting and version of the C ABI (host only).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/omf_codec.h"
#include "omf_common.h"

namespace omf {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

int hip_fail(hipError_t e, const char* what) {
  g_last_error = std::string(what) + ": " + hipGetErrorString(e);
  return OMF_EHIP;
}

}  // namespace omf

extern "C" {

int omf_abi_version(void) { return OMF_ABI_VERSION; }

const char* omf_last_error(void) { return omf::g_last_error.c_str(); }

int omf_host_alloc(size_t nbytes, void** out) {
  if (!out) return omf::fail(OMF_EINVAL, "omf_host_alloc: out is NULL");
  *out = nullptr;
  if (nbytes == 0) return omf::fail(OMF_EINVAL, "omf_host_alloc: nbytes is 0");
  const hipError_t e = hipHostMalloc(out, nbytes, hipHostMallocDefault);
  if (e == hipSuccess) return OMF_OK;
  *out = nullptr;
  (void)hipGetLastError();  // reported here, not by the caller's next launch
  if (e == hipErrorOutOfMemory) return omf::fail(OMF_ENOMEM, "omf_host_alloc: out of page-locked memory");
  return omf::hip_fail(e, "hipHostMalloc");
}

int omf_host_free(void* ptr) {
  if (!ptr) return OMF_OK;
  OMF_HIP(hipHostFree(ptr));
  return OMF_OK;
}

}  // extern "C"
