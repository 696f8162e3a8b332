// Why an entry point refused its arguments: the C-ABI returns hipErrorInvalidValue, the reason is kept per host thread.
// Beside it, per host thread as well: what the last call of every fused family launched (icrl_debug_last_route).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "common.h"

namespace icrl {

static thread_local char g_last_error[512] = "";

int fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_last_error, sizeof(g_last_error), fmt, ap);
  va_end(ap);
  return (int)hipErrorInvalidValue;
}

// eight words per family (ICRL_FAMILY_*).  Host state only: no kernel reads it and no launch depends on it.
static thread_local int32_t g_route[ICRL_N_FAMILIES][8] = {};

void note_route(int family, int w0, int w1, int w2, int w3, int w4, int w5, int w6, int w7) {
  if (family < 0 || family >= ICRL_N_FAMILIES) return;
  const int32_t w[8] = {w0, w1, w2, w3, w4, w5, w6, w7};
  memcpy(g_route[family], w, sizeof(w));
}

}  // namespace icrl

extern "C" int icrl_debug_last_route(int family, int32_t* out8) {
  if (family < 0 || family >= ICRL_N_FAMILIES) return icrl::fail("icrl_debug_last_route: family %d (0 rollout, 1 update, 2 GAE)", family);
  if (out8 == nullptr) return icrl::fail("icrl_debug_last_route: out8 is NULL (8 int32 are written)");
  memcpy(out8, icrl::g_route[family], sizeof(icrl::g_route[family]));
  return 0;
}

extern "C" const char* icrl_last_error(void) { return icrl::g_last_error; }
extern "C" void icrl_clear_error(void) { icrl::g_last_error[0] = 0; }
