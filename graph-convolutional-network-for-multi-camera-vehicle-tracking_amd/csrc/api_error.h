// The error text of the C ABI (mtmc_mpn_last_error, include/mtmc_mpn.h): one buffer per host thread, written by every
// entry point that returns a negative code.  An `extern "C"` function leaves through fail(...) or launched(...), and its
// message starts with its own name without the mtmc_ prefix.
#pragma once
#include "../../include/mtmc_mpn.h"

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

namespace mtmc_api {

inline thread_local char g_err[512] = "";

inline int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// the end of an entry point that launched kernels: MTMC_OK, or what HIP says went wrong with a launch
inline int launched(const char* entry) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MTMC_OK : fail(MTMC_E_HIP, "%s: kernel launch failed: %s", entry, hipGetErrorString(e));
}

}  // namespace mtmc_api
