// TEST INFRASTRUCTURE (tests/test_inverse_waves_cpu.py): which inverse calls the planner marks PLAIN -- the ones
// vw_inv.hip may run through k_inverse_seq's PLAIN form at VW_INV_WAVES = 6 | 8 -- as a host program over
// vw_plan.cpp.  Prints one line per case: name kernel full plain waves.
#include <cstdint>
#include <cstdio>
#include "vw_plan.h"

using namespace vw;

template <typename T>
static InvCall<T> headline() {
  InvCall<T> c;
  c.details = reinterpret_cast<const T*>(uintptr_t(0x10000));  // aligned, never dereferenced by the planner
  c.approx = reinterpret_cast<const T*>(uintptr_t(0x20000));
  c.y = reinterpret_cast<T*>(uintptr_t(0x30000));
  c.B = 4096; c.N = 4096; c.L = 8; c.J = 6;
  c.boundary = VW_PERIODIC;
  c.flags = VW_FLAG_FMA;
  return c;
}

template <typename T>
static void show(const char* name, const Tuning& tu, const InvCall<T>& c) {
  InvPlan<T> p;
  plan_inverse(tu, c, &p);
  const char* k = !p.fused ? "levels" : p.kernel == kInvSeq ? "seq" : p.kernel == kInvDb ? "db" : "other";
  printf("%s %s full=%d plain=%d waves=%d\n", name, k, p.args.full, p.args.plain, p.args.waves);
}

int main() {
  Tuning d, w8, w8b1;
  set_tuning(w8, "VW_INV_WAVES", 8);
  set_tuning(w8b1, "VW_INV_WAVES", 8);
  set_tuning(w8b1, "VW_INV_BUF", 1);
  const double thr = 0;

  show("default", d, headline<double>());
  show("waves8", w8, headline<double>());
  { Tuning t; set_tuning(t, "VW_INV_WAVES", 7); show("waves7", t, headline<double>()); }
  { auto c = headline<double>(); c.flags = 0; show("exact", w8, c); }
  { auto c = headline<double>(); c.N = 512; c.B = 5; show("small_db", w8, c); show("small_seq", w8b1, c); }
  { auto c = headline<double>(); c.N = 1024; c.J = 7; c.B = 5; show("n1024_j7", w8b1, c); }
  { auto c = headline<double>(); c.N = 512; c.J = 4; c.B = 5; c.thr = &thr; show("threshold", w8b1, c); }
  { auto c = headline<double>(); c.N = 512; c.J = 4; c.B = 5; c.boundary = VW_SYMMETRIC; show("symmetric", w8b1, c); }
  { auto c = headline<double>(); c.N = 500; c.J = 3; c.B = 5; show("ragged", w8b1, c); }
  { auto c = headline<double>(); c.approx_zero = 1; show("approx_zero", w8, c); }
  { auto c = headline<double>(); c.detail_mask = ~2u; show("masked_level", w8, c); }
  { auto c = headline<double>(); c.flags |= VW_FLAG_REF_NONFINITE; show("ref_nonfinite", w8, c); }
  { Tuning t = w8; set_tuning(t, "VW_INV_REV", 1); show("reverse_walk", t, headline<double>()); }
  { Tuning t = w8; set_tuning(t, "VW_LEVEL_CT", 0); show("level_ct0", t, headline<double>()); }
  { auto c = headline<double>(); c.y = reinterpret_cast<double*>(uintptr_t(0x30008)); show("misaligned", w8, c); }
  { auto c = headline<double>(); c.L = 16; show("taps16", w8, c); }
  show("fp32", w8, headline<float>());
  return 0;
}
