// Library-wide state of libmink_hip.so: the thread-local error text behind MINK_REQUIRE / MINK_HIP (common.h) and the ABI
// version.  Every other translation unit links against this one for set_error.  No kernel lives here.
#include "common.h"

namespace mink {

static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}

}  // namespace mink

extern "C" {

const char *mink_last_error(void) { return mink::g_err; }
int mink_abi_version(void) { return MINK_ABI_VERSION; }

}  // extern "C"
