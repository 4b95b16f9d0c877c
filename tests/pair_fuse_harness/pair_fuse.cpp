// TEST INFRASTRUCTURE (tests/test_pair_fuse_cpu.py): which forward -> inverse pairs the planner's pair_fusable accepts
// for the round-trip kernel (vw_pair.hip), as a host program over vw_plan.cpp.  Prints one line per case: name 0|1.
#include <cstdint>
#include <cstdio>
#include "vw_plan.h"

using namespace vw;

template <typename T>
struct Pair {
  FwdCall<T> f;
  InvCall<T> i;
};

// the headline pair: db4, J = 6, 4096 x 4096, FMA; pointers aligned and apart, never dereferenced by the planner
template <typename T>
static Pair<T> headline() {
  Pair<T> p;
  const uintptr_t gib = uintptr_t(1) << 30;
  p.f.x = reinterpret_cast<const T*>(1 * gib);
  p.f.details = reinterpret_cast<T*>(2 * gib);
  p.f.approx = reinterpret_cast<T*>(4 * gib);
  p.f.B = 4096; p.f.N = 4096; p.f.ldx = 4096; p.f.L = 8; p.f.J = 6;
  p.f.boundary = VW_PERIODIC; p.f.flags = VW_FLAG_FMA;
  p.i.details = p.f.details; p.i.approx = p.f.approx;
  p.i.y = reinterpret_cast<T*>(5 * gib);
  p.i.B = 4096; p.i.N = 4096; p.i.L = 8; p.i.J = 6;
  p.i.boundary = VW_PERIODIC; p.i.flags = VW_FLAG_FMA;
  return p;
}

template <typename T>
static void show(const char* name, const Tuning& tu, const Pair<T>& c) {
  FwdPlan<T> fp;
  InvPlan<T> ip;
  plan_forward(tu, c.f, &fp);
  plan_inverse(tu, c.i, &ip);
  printf("%s %d\n", name, pair_fusable(c.f, fp, c.i, ip) ? 1 : 0);
}

template <typename T, typename F>
static void with(const char* name, F&& change, const Tuning& tu = Tuning()) {
  Pair<T> c = headline<T>();
  change(c);
  show(name, tu, c);
}

int main() {
  using P = Pair<double>;
  const double thr = 0;
  with<double>("headline", [](P&) {});
  with<double>("exact", [](P& c) { c.f.flags = c.i.flags = 0; });
  with<double>("n512", [](P& c) { c.f.N = c.f.ldx = c.i.N = 512; c.f.B = c.i.B = 4096; });
  with<double>("n512_small_batch", [](P& c) { c.f.N = c.f.ldx = c.i.N = 512; c.f.B = c.i.B = 3; });
  with<double>("n512_j7", [](P& c) { c.f.N = c.f.ldx = c.i.N = 512; c.f.J = c.i.J = 7; });
  with<double>("haar_j1", [](P& c) { c.f.L = c.i.L = 2; c.f.J = c.i.J = 1; });
  // one case per reason to stay two kernels
  with<double>("other_details", [](P& c) { c.i.details = reinterpret_cast<const double*>(uintptr_t(7) << 30); });
  with<double>("other_approx", [](P& c) { c.i.approx = reinterpret_cast<const double*>(uintptr_t(7) << 30); });
  with<double>("masked_level", [](P& c) { c.i.detail_mask = ~2u; });
  with<double>("approx_zero", [](P& c) { c.i.approx_zero = 1; });
  with<double>("ref_nonfinite", [](P& c) { c.f.flags |= VW_FLAG_REF_NONFINITE; c.i.flags |= VW_FLAG_REF_NONFINITE; });
  with<double>("validate", [](P& c) { c.f.flags |= VW_FLAG_VALIDATE; });
  with<double>("host_memory", [](P& c) { c.i.flags |= VW_FLAG_HOST_MEMORY; });
  with<double>("threshold", [&](P& c) { c.i.thr = &thr; });
  with<double>("y_is_x", [](P& c) { c.i.y = const_cast<double*>(c.f.x); });
  with<double>("y_in_details", [](P& c) { c.i.y = c.f.details + 5 * 4096 * 4096; });
  with<double>("symmetric", [](P& c) { c.f.boundary = c.i.boundary = VW_SYMMETRIC; });
  with<double>("mixed_modes", [](P& c) { c.i.flags = 0; });
  with<double>("other_batch", [](P& c) { c.i.B = 2048; });
  with<double>("other_levels", [](P& c) { c.i.J = 5; });
  with<double>("sym8", [](P& c) { c.f.L = c.i.L = 16; });
  with<double>("n4100", [](P& c) { c.f.N = c.f.ldx = c.i.N = 4100; });
  with<double>("padded_rows", [](P& c) { c.f.ldx = 4100; });  // x rows apart but 16-byte aligned: still one launch
  { Tuning t; set_tuning(t, "VW_LEVEL_CT", 0); with<double>("level_ct0", [](P&) {}, t); }
  { Tuning t; set_tuning(t, "VW_FWD_PERSIST", 0); with<double>("no_persist", [](P&) {}, t); }
  { Tuning t; set_tuning(t, "VW_INV_REV", 1); with<double>("reverse_walk", [](P&) {}, t); }
  with<float>("fp32", [](Pair<float>&) {});
  return 0;
}
