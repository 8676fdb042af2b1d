// mb_options.cpp -- the override table behind mb_set_option and the lookups over the option table of mb_options.h.
// Plain host C++: no HIP, and nothing of the rest of the library.
#include "mb_options.h"

#include <cstdio>
#include <cstring>
#include <string>

namespace mb {

// mb_set_option keeps its values here: the process environment is the host's, not the library's to write.  A function-local
// static, so that a read made while the library loads (MB_JIT_MAXCANDS) finds a constructed object whatever the link order.
// Readers run inside API calls, under the API lock.
struct Override { bool set = false; std::string value; };
static Override *overrides() {
  static Override table[OPT_COUNT];
  return table;
}

const char *opt_raw(Opt id) {
  const Override &o = overrides()[id];
  return o.set ? o.value.c_str() : getenv(OPT_TABLE[id].name);
}

void opt_override(Opt id, const char *value) {
  Override &o = overrides()[id];
  o.set = value && *value;
  o.value = o.set ? value : "";
}

int opt_find(const char *name) {
  if (name)
    for (int k = 0; k < OPT_COUNT; ++k) if (strcmp(name, OPT_TABLE[k].name) == 0) return k;
  return -1;
}

const char *opt_list() {
  static const std::string text = []() {
    std::string s;
    for (const OptEntry &e : OPT_TABLE) {
      char dflt[32] = "-";
      if (e.dflt == OPT_BY_CALL) snprintf(dflt, sizeof dflt, "by call");
      else if (e.dflt != OPT_NONE) snprintf(dflt, sizeof dflt, "%.10g", e.dflt);
      s += std::string(e.name) + "\t" + e.kindName + "\t" + dflt + "\t" + e.clsName + "\t" + e.note + "\n";
    }
    return s;
  }();
  return text.c_str();
}

}  // namespace mb
