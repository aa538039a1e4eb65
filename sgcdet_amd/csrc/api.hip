// Introspection, error plumbing and the tuning knobs of the gfx950 library (include/sgcdet_amd.h).
#include <stdarg.h>

#include <string.h>

#include "common.hpp"
#include "tuning.hpp"

namespace sgc {
#define SGC_KNOB_DEFINE(key, var, def, doc) int var = def;
SGC_TUNING_KNOBS(SGC_KNOB_DEFINE)
#undef SGC_KNOB_DEFINE

static thread_local char g_err[512] = "";

int set_error(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace sgc

extern "C" int sgc_abi_version(void) { return SGC_ABI_VERSION; }
extern "C" const char *sgc_last_error(void) { return sgc::g_err; }
extern "C" const char *sgc_backend(void) { return "hip-gfx950"; }

extern "C" int sgc_set_tuning(const char *key, int value) {
  static const struct { const char *key; int *var; } knobs[] = {
#define SGC_KNOB_ENTRY(key, var, def, doc) {key, &sgc::var},
      SGC_TUNING_KNOBS(SGC_KNOB_ENTRY)
#undef SGC_KNOB_ENTRY
  };
  if (!key) return sgc::set_error(SGC_EINVAL, "sgc_set_tuning: null key");
  for (const auto &k : knobs)
    if (!strcmp(key, k.key)) {
      const bool positive = k.var == &sgc::g_tune_split_min_steps || k.var == &sgc::g_tune_split_max;
      *k.var = positive && value < 1 ? 1 : value;
      return SGC_OK;
    }
  return sgc::set_error(SGC_EINVAL, "sgc_set_tuning: unknown key %s", key);
}
