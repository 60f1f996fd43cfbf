// Host code only: the one place that reads the walk and launcher switches from the environment (walk_knobs.h).  No __global__ code and no
// HIP call in this file.
#include "walk_knobs.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

namespace dfh {

namespace {
bool off_at_0(const char* e, bool) { return !(e && e[0] == '0'); }
bool on_at_1(const char* e, bool) { return e && e[0] == '1'; }
int as_int(const char* e, int dflt) { return e ? atoi(e) : dflt; }
double as_double(const char* e, double dflt) { return e ? atof(e) : dflt; }

void put(std::string& s, const char* name, bool v) { s += name; s += v ? "=1\n" : "=0\n"; }
void put(std::string& s, const char* name, int v) { s += name; s += '='; s += std::to_string(v); s += '\n'; }
void put(std::string& s, const char* name, double v) { char b[32]; snprintf(b, sizeof(b), "=%g\n", v); s += name; s += b; }
}  // namespace

const WalkKnobs& WalkKnobs::get() {
  static const WalkKnobs knobs = [] {
    WalkKnobs k;
#define DFH_X(type, field, name, parse, dflt) k.field = parse(getenv(#name), dflt);
    DFH_WALK_KNOBS(DFH_X)
#undef DFH_X
    return k;
  }();
  return knobs;
}

size_t walk_switches_text(char* buf, size_t cap) {
  const WalkKnobs& k = WalkKnobs::get();
  std::string s;
#define DFH_X(type, field, name, parse, dflt) put(s, #name, k.field);
  DFH_WALK_KNOBS(DFH_X)
#undef DFH_X
  if (buf && cap) {
    const size_t n = s.size() < cap - 1 ? s.size() : cap - 1;
    memcpy(buf, s.data(), n);
    buf[n] = 0;
  }
  return s.size();
}

}  // namespace dfh
