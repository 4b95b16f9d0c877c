// vw_plan.cpp -- kernel selection (vw_plan.h): level bookkeeping restated from the reference, policy, LDS
// layout arithmetic.  Host-only: no HIP call, no allocation on the device, no dereference of a caller's pointer.
#include "vw_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace vw {

// ------------------------------------------------------------------------------------------------
// The tuning switches by name: clamping per switch, value < 0 = the default (d).  read_tuning scans the
// environment in this order (VW_DEEP before VW_DEEP_INV: the narrower switch wins).
struct TuningKey {
  const char* name;
  void (*set)(Tuning& t, const Tuning& d, int v);
};
#define VW_KEY(name, stmt) {name, [](Tuning& t, const Tuning& d, int v) { (void)d; stmt; }}
static const TuningKey kTuningTable[] = {
    VW_KEY("VW_NV", t.nv = v < 0 ? d.nv : v <= 4 ? 4 : 8),
    VW_KEY("VW_FWD_PERSIST", t.fwd_persist = v < 0 ? d.fwd_persist : v != 0),
    VW_KEY("VW_FWD_BUF", t.fwd_buf = v < 0 ? d.fwd_buf : v),
    VW_KEY("VW_FORCE_TILED", t.force_tiled = v > 0),
    VW_KEY("VW_FWD_REV", t.fwd_rev = v < 0 ? 0 : v),
    VW_KEY("VW_INV_REV", t.inv_rev = v < 0 ? 0 : v),
    VW_KEY("VW_FWD_TILE", t.fwd_tile = v < 0 ? 0 : v),
    VW_KEY("VW_MULTI", t.multi = v < 0 ? d.multi : v != 0),
    VW_KEY("VW_MULTI_DIV", t.multi_div = v <= 0 ? d.multi_div : v),
    VW_KEY("VW_MULTI_TILE", t.multi_tile = v < 0 ? 0 : v),
    VW_KEY("VW_INV_BUF", t.inv_buf = v < 0 ? 0 : v),  // 0 = policy
    VW_KEY("VW_INV_TILE", t.inv_tile = v < 0 ? 0 : v),
    VW_KEY("VW_MULTI_RBLK", t.multi_rblk = v < 0 ? d.multi_rblk : v),
    VW_KEY("VW_MULTI_PF", t.multi_pf = v < 0 ? d.multi_pf : v),
    VW_KEY("VW_MULTI_PAD", t.multi_pad = v < 0 ? d.multi_pad : v),
    VW_KEY("VW_MULTI_INV_TILE", t.multi_inv_tile = v < 0 ? 0 : v),
    VW_KEY("VW_NO_SWEEP", t.no_sweep = v > 0),
    VW_KEY("VW_SWEEP_QC", t.sweep_qc = v >= 16 ? v : d.sweep_qc),
    VW_KEY("VW_UNROLL_MAX", t.unroll_max = v < 0 ? d.unroll_max : v),
    VW_KEY("VW_BLK", t.blk = v < 0 ? d.blk : v),
    VW_KEY("VW_FWD_NV", t.fwd_nv = v < 0 ? d.fwd_nv : v),
    VW_KEY("VW_INV_NV", t.inv_nv = v < 0 ? d.inv_nv : v),
    VW_KEY("VW_DEEP", t.deep = v < 0 ? d.deep : v != 0; t.deep_inv = v < 0 ? d.deep_inv : v != 0),
    VW_KEY("VW_DEEP_INV", t.deep_inv = v < 0 ? d.deep_inv : v != 0),
    VW_KEY("VW_DEEP_LDS", t.deep_lds = v <= 0 ? d.deep_lds : v),
    VW_KEY("VW_DEEP_WAVES", t.deep_waves = v <= 0 ? d.deep_waves : v),
    VW_KEY("VW_DEEP_PF_FWD", t.deep_pf_fwd = v <= 0 ? d.deep_pf_fwd : std::min(v, 16)),
    VW_KEY("VW_DEEP_PF_INV", t.deep_pf_inv = v <= 0 ? d.deep_pf_inv : std::min(v, 16)),
    VW_KEY("VW_SWEEP2", t.sweep2 = v < 0 ? d.sweep2 : v),
    VW_KEY("VW_SWEEP2_KA", t.sweep2_ka = v == 16 ? 16 : v == 8 ? 8 : d.sweep2_ka),
    VW_KEY("VW_SWEEP2_UC", t.sweep2_uc = v >= 32 ? v : d.sweep2_uc),
    VW_KEY("VW_SWEEP2_R", t.sweep2_r = v == 32 ? 32 : 0),
    VW_KEY("VW_SWEEP2_MINB", t.sweep2_minb = v < 0 ? d.sweep2_minb : v),
    VW_KEY("VW_BLK_FWD8", t.blk_fwd8 = v < 0 ? d.blk_fwd8 : v),
    VW_KEY("VW_DMA_NT", t.dma_nt = v < 0 ? d.dma_nt : v),
    VW_KEY("VW_MULTI_NI", t.multi_ni = v < 0 ? d.multi_ni : v == 4 ? 4 : 8),
    VW_KEY("VW_MFMA", t.mfma = v < 0 ? d.mfma : v),
    VW_KEY("VW_REF_GRID", t.ref_grid = v < 0 ? d.ref_grid : v),
    VW_KEY("VW_LEVEL_CT", t.level_ct = v < 0 ? d.level_ct : v != 0),
    VW_KEY("VW_ENERGY_FUSED", t.energy_fused = v < 0 ? d.energy_fused : v),
    VW_KEY("VW_MRA_FUSED", t.mra_fused = v < 0 ? d.mra_fused : v >= 2 ? 2 : v),
    VW_KEY("VW_BI", t.bi = v < 0 ? d.bi : v & 7),
    VW_KEY("VW_BI_LISTED", t.bi_listed = v < 0 ? d.bi_listed : v != 0),
    VW_KEY("VW_INV_WAVES", t.inv_waves = v == 6 || v == 8 ? v : d.inv_waves),
    VW_KEY("VW_PAIR_FUSE", t.pair_fuse = v < 0 ? d.pair_fuse : v != 0),
    VW_KEY("VW_PAIR_KEEP", t.pair_keep = v < 0 ? d.pair_keep : std::min(v, kPairMaxKeep)),
};
#undef VW_KEY

bool set_tuning(Tuning& t, const char* key, int v) {
  const Tuning d;
  for (const TuningKey& k : kTuningTable)
    if (!strcmp(k.name, key)) { k.set(t, d, v); return true; }
  return false;
}

Tuning read_tuning() {
  Tuning t;
  const Tuning d;
  for (const TuningKey& k : kTuningTable) {
    const char* e = getenv(k.name);
    // presence-style switches (VW_FORCE_TILED, VW_NO_SWEEP) are on when set to anything but "0"
    if (e) k.set(t, d, *e == '\0' ? 1 : atoi(e));
  }
  return t;
}

// ------------------------------------------------------------------------------------------------
// Bookkeeping restated from the reference.

// MultiLevelMODWTTransform.calculateMaxLevels  core/modwt/MultiLevelMODWTTransform.java:455-501
int max_levels(int64_t N, int L) {
  if (L <= 0 || N <= L) return 0;
  int max_level = 1;
  const long long lm1 = L - 1;
  while (max_level < 10) {
    const long long scaled = lm1 * (1LL << (max_level - 1)) + 1LL;
    if (scaled > N) break;
    max_level++;
  }
  return max_level - 1;
}

int64_t upsampled_length(int L, int level) {
  const int64_t up = (level <= 1) ? 1 : ((int64_t)1 << (level - 1));
  return (int64_t)(L - 1) * up + 1;
}

int ref_mode(int boundary) {
  return boundary == VW_PERIODIC ? kHaloPeriodic : boundary == VW_ZERO_PADDING ? kHaloZero : kHaloSymmetric;
}

// SymmetricAlignmentStrategy.decide  core/modwt/SymmetricAlignmentStrategy.java:43-117
static void sym_decide(int wid, int L, int level, int* ap, int* dh, int* dp, int* dg) {
  int detailPlus = 1, deltaG = 0, deltaH = 0;
  const bool isHaar = L <= 2;
  int approxPlus = isHaar ? 1 : 0;
  if (isHaar) {
    deltaG = 0;
    deltaH = (level <= 1) ? 0 : -1;
  } else if (wid == VW_WID_DB6) {
    deltaH = (level <= 1) ? 0 : -1;
    deltaG = (level >= 3) ? 1 : 0;
  } else if (wid == VW_WID_DB8) {
    deltaH = (level <= 1) ? 0 : 1;
    deltaG = (level >= 2) ? 1 : 0;
  } else if (wid == VW_WID_SYM4) {
    approxPlus = 1; detailPlus = 0; deltaH = 0; deltaG = 0;
  } else if (wid == VW_WID_SYM8) {
    if (level <= 1) { deltaH = 0; deltaG = 0; }
    else if (level == 2) { deltaH = 1; deltaG = 0; }
    else { deltaH = 1; deltaG = 1; }
  } else if (wid == VW_WID_COIF2) {
    approxPlus = 1; deltaH = (level <= 1) ? 0 : 1; detailPlus = 0; deltaG = 0;
  } else if (wid == VW_WID_COIF3) {
    detailPlus = 0;
    if (level <= 1) { deltaH = 0; deltaG = 0; } else { deltaH = -1; deltaG = 1; }
  } else if (L >= 12) {
    if (level <= 1) { deltaH = 0; deltaG = 0; }
    else { const bool even = level % 2 == 0; deltaH = even ? 0 : -1; deltaG = even ? 0 : -1; }
  } else {
    if (level <= 1) { deltaH = 0; deltaG = 0; } else { deltaH = -1; deltaG = 0; }
  }
  *ap = approxPlus; *dh = deltaH; *dp = detailPlus; *dg = deltaG;
}

// MultiLevelMODWTTransform.computeTauJ  core/modwt/MultiLevelMODWTTransform.java:795-806
static int compute_tau(int base_len, int level) {
  const int lm1 = base_len - 1;
  if (level <= 1) return std::max(0, lm1 / 2);
  const long long up = 1LL << (level - 1);
  const long long Lj = (long long)lm1 * up + 1LL;
  const long long tau = (Lj - 1LL) / 2LL;
  if (tau < 0) return 0;
  if (tau > 2147483647LL) return 2147483647;
  return (int)tau;
}

static int next_pow2(int64_t n) {
  int64_t p = 1;
  while (p < n) p <<= 1;
  return (int)p;
}

static bool is_pow2(int64_t n) { return n > 0 && (n & (n - 1)) == 0; }

// Level-j input index range read by a branch (dir, off) for outputs t in [0, tmax].
static void branch_extent(int N, int tmax, int L, int s, int dir, int off, int* hl, int* hr) {
  const long long reach = (long long)(L - 1) * s;
  long long mn, mx;
  if (dir > 0) { mn = off; mx = (long long)tmax + reach + off; }
  else { mn = (long long)off - reach; mx = (long long)tmax + off; }
  *hl = (int)std::max<long long>(*hl, -mn);
  *hr = (int)std::max<long long>(*hr, mx - (N - 1));
}

static inline int64_t round_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
template <typename T> static constexpr int vec_width() { return 16 / (int)sizeof(T); }
static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
static bool plus_zero(const LevelDesc& d) { return d.dir_a == 1 && d.dir_d == 1 && d.off_a == 0 && d.off_d == 0; }

// Alignment of the buffers a per-level step names: the caller's by their pointers, the workspace halves by
// the plane size (the base comes from hipMalloc: 256-byte aligned), plane k of the details by both.
struct StepAlign {
  const void* in;
  const void* out;
  const void* planes;
  size_t plane_bytes;
  bool buf(int b) const {
    return b == kBufIn ? aligned16(in) : b == kBufOut ? aligned16(out) : b == kBufWs1 ? plane_bytes % 16 == 0 : true;
  }
  bool plane(int k) const { return (((uintptr_t)planes + (uintptr_t)k * plane_bytes) & 15u) == 0; }
};

template <typename P>
static void plan_error(P* p, int code, const char* fmt, int a = 0, int b = 0) {
  p->error = code;
  snprintf(p->msg, sizeof(p->msg), fmt, a, b);
}

// ------------------------------------------------------------------------------------------------
// Plan of a fused launch: threads, vectors per thread (4 or 8), LDS bytes.  NV = 4 keeps the
// per-thread register arrays small (no spills); NV = 8 reaches N = 1024 * 8 * V.  The workgroup is
// ceil(nvec / NV) threads (not rounded to a wave): thread `tid` owns vectors tid + k*threads, and
// the unrolled kernels rely on slabs 0..NV-2 being full, `fit` = (NV-1)*threads <= nvec (else the
// runtime-L kernel with a bounds check per vector runs).
static bool fused_plan(const Tuning& tu, int64_t N, int V, int elem, int64_t lds_elems_extra, int* threads, int* nv,
                       int* lds, bool* fit, int nv_req = 0) {
  const int64_t nvec = (N + V - 1) / V;
  int want = tu.nv;
  if ((nvec + want - 1) / want > 512) want = 8;  // NV = 4 kernels are bounded to 512 threads (VW_FUSED_BOUNDS)
  // NV = 2: 1024 threads at most, every slab full (the unrolled kernels' contract)
  if (nv_req == 2 && nvec % 2 == 0 && nvec / 2 <= kMaxThreads) want = 2;
  const int64_t th = (nvec + want - 1) / want;
  if (th > kMaxThreads) return false;
  const int64_t bytes = lds_elems_extra * elem;
  if (bytes > kLdsBytes) return false;
  *nv = want;
  *threads = (int)th;
  *lds = (int)bytes;
  *fit = (int64_t)(want - 1) * th <= nvec;
  return true;
}

// Owner-written halo of one level (vw_dev_core.h halo_images): the affine images of an element and
// the vector bands that have them; `own` only when every band lies in the slab that checks it.
static void set_halo_images(LevelDesc& d, int64_t N, int64_t npow2, int V, int threads, int nv) {
  int64_t s_el = 0, e_el = N;
  d.il_a = 0; d.il_b = 1; d.ir_a = 0; d.ir_b = -1;  // no images
  switch (d.mode) {
    case kHaloPeriodic:
      d.il_a = 1; d.il_b = (int)-N; d.ir_a = 1; d.ir_b = (int)N;
      s_el = d.hr; e_el = N - d.hl;
      break;
    case kHaloSymmetric:
      d.il_a = -1; d.il_b = -1; d.ir_a = -1; d.ir_b = (int)(2 * N - 1);
      s_el = d.hl; e_el = N - d.hr;
      break;
    case kHaloFftPad:
      d.il_a = 1; d.il_b = (int)-npow2;
      e_el = npow2 - d.hl;
      break;
    default:
      break;
  }
  e_el = std::min<int64_t>(std::max<int64_t>(e_el, 0), N);
  d.vs = (int)((s_el + V - 1) / V);
  d.ve = (int)(e_el / V);
  d.own = (d.hl <= N && d.hr <= N && d.vs <= threads && (int64_t)d.ve >= (int64_t)(nv - 1) * threads) ? 1 : 0;
}

// Padded LDS layout of the register-blocked PERIODIC kernels (vw_blk.h k_forward_blk / k_inverse_blk),
// one rule for both directions.  The forward keeps one left halo for all levels (whole pad groups of 16
// vectors where they fit: the kernel then reads at wave-uniform (NV = 8) or compile-time (NV = 4) offsets);
// the inverse a right halo per level.  `ok`: every level PERIODIC in the +1 / 0 orientation, the rows
// divide into blocks of NV * m_J vectors, the halo lies within the row and the buffer (inverse: + tap table) fits LDS.
// `tight`: sparse padding (blk_pad) so that an NV = 8 level fits (sym8 at N = 16384); the forward
// reports it even where the layout is not used, as its argument struct always has.
struct BlkPlan {
  bool ok;
  int tight;
  int64_t buf;  // vectors per level buffer
  int hlv;      // forward: vectors of left halo
};
template <typename T>
static BlkPlan blk_plan(const LevelDesc* lv, int J, int L, int64_t nvec, int nv, bool inverse) {
  constexpr int V = vec_width<T>();
  const int64_t taps_b = 2 * L * (int64_t)sizeof(T);
  const int mJ = std::max(1, lv[J - 1].s / V);
  BlkPlan r{nvec % ((int64_t)nv * mJ) == 0, 0, 0, 0};
  int64_t halo[kMaxLevels], hmax = 0;
  for (int j = 0; j < J; ++j) {
    if (inverse ? !plus_zero(lv[j]) : lv[j].mode != kHaloPeriodic) r.ok = false;
    halo[j] = ((int64_t)(L - 1) * lv[j].s + V - 1) / V;
    hmax = std::max(hmax, halo[j]);
  }
  if (!inverse && round_up(hmax, 16) <= nvec) hmax = round_up(hmax, 16);
  if (hmax > nvec) r.ok = false;
  int64_t buf[2] = {0, 0};
  for (int j = 0; j < J; ++j)
    for (int tight = 0; tight < 2; ++tight) {
      const BlkLayout lo = blk_pad(lv[j].s / V, nv, tight);
      const int64_t u = nvec + (inverse ? halo[j] : hmax) - 1;
      buf[tight] = std::max(buf[tight], u + (u >> lo.sh) * lo.pad + 1);
    }
  const bool roomy = buf[0] * 16 + taps_b <= kLdsBytes;
  r.tight = (nv >= 8 && !roomy && (!inverse || (r.ok && buf[1] * 16 + taps_b <= kLdsBytes))) ? 1 : 0;
  r.buf = buf[r.tight];
  r.hlv = (int)hmax;
  // (the forward has always tested the buffer alone here and the tap table at its launch size)
  r.ok = r.ok && r.buf * 16 + (inverse ? taps_b : 0) <= kLdsBytes;
  return r;
}

// fp32 FMA, PERIODIC, long filters: the matrix-core kernels (vw_mfma.hip, VW_MFMA).  Returns the LDS
// bytes (0 = not eligible) and the halo / padded region of the level row; `scratch` floats follow the
// region and the taps (the forward's per-wave transpose scratch).
static int mfma_layout(bool ok, int L, int J, int64_t N, int scratch, int* halo, int* region) {
  if (!ok || !mfma_supported(L, N)) return 0;
  const int H = mfma_halo(L, J);
  const int reg = mfma_region((int)N + H);  // padded LDS layout (vw_mfma.hip ph)
  if (H > N || (int64_t)(reg + 2 * L + scratch) * 4 > kLdsBytes) return 0;
  *halo = H;
  *region = reg;
  return (reg + 2 * L + scratch) * 4;
}

// Level groups of the per-level path (vw_dev_lvl.h k_forward_multi / k_inverse_multi): from level 1
// up, consecutive PERIODIC levels run as one multi-level tile launch while their combined reach
// sum((L-1)*s_j) stays within a quarter of the tile (the redundant arithmetic).  g[j-1] = size
// of the group starting at level j (0 inside a group, 1 = the per-level kernels).  VW_MULTI=0
// disables; VW_MULTI_TILE / VW_MULTI_DIV tune tile and reach bound.
template <typename T>
static int multi_tile(const Tuning& tu) {
  constexpr int V = vec_width<T>();
  const int v = tu.multi_tile ? tu.multi_tile : (int)(16384 / sizeof(T));
  return v >= 64 * V ? v / V * V : 64 * V;
}

static void level_groups(const Tuning& tu, const LevelDesc* lv, int J, int L, int V, int tile, bool ok, int* g) {
  std::fill(g, g + J, 1);
  if (!ok || !tu.multi) return;
  const int64_t cap = tile / tu.multi_div;
  for (int j = 1; j <= J;) {
    int n = 0;
    int64_t ext = 0;
    while (j + n <= J && n < kMaxGroup && lv[j + n - 1].mode == kHaloPeriodic) {
      const int64_t e2 = ext + round_up((int64_t)(L - 1) * lv[j + n - 1].s, V);
      if (e2 > cap) break;
      ext = e2;
      ++n;
    }
    if (n >= 2) {
      g[j - 1] = n;
      for (int k = 1; k < n; ++k) g[j - 1 + k] = 0;
      j += n;
    } else {
      ++j;
    }
  }
}

// Level group of the chained column sweeps (vw_dev_lvl.h k_inverse_sweep2 / k_inverse_sweep3): inverse levels
// j .. j-levels+1 (spacings G*h .. h, G = 2 / 4), all column-sweep levels outside the multi-level tile
// groups, PERIODIC / dir +1 / offset 0.  Picks KA (outputs per thread and step) and R (residues per
// group, 64 or 32 = h's alignment) under the kernels' rules: a block of G*KA positions covers the
// reach of the levels below the top (L-1 per level, in the bottom level's positions: 1 / 2 steps), the
// LDS rings (1 / 2 of 3 blocks x R) fit, one wrap mod N at most, and residue classes of >= 64 blocks.
template <typename T>
static bool sweepg_plan(const Tuning& tu, const LevelDesc* lv, int j, int levels, int L, int64_t N,
                        const char* in_group, const int* start_of, int* ka_out, int* r_out) {
  if (levels < 2 || levels > 3 || j < levels) return false;
  const int G = levels == 2 ? 2 : 4;
  const int64_t h = lv[j - levels].s;
  if (h < kSweepMinS || h % 32 != 0 || lv[j - 1].s != G * h) return false;
  for (int k = j - levels + 1; k <= j; ++k) {
    if (lv[k - 1].mode != kHaloPeriodic || !plus_zero(lv[k - 1])) return false;
    if (k < j && (in_group[k] || start_of[k] != 0)) return false;
  }
  const int R = (h % 64 == 0 && tu.sweep2_r != 32) ? 64 : 32;
  const int kmin = (levels == 2 ? 1 : 2) * (L - 1);
  for (int ka : {L <= 17 ? tu.sweep2_ka : 16, 16}) {
    for (int r : {R, 32}) {
      const int64_t kb = (int64_t)G * ka;
      const int64_t lds = (levels == 2 ? 1 : 2) * 3 * kb * r * (int64_t)sizeof(T);
      if (kb < kmin || lds > kLdsBytes || h % r != 0) continue;
      if (N % (G * h) != 0 || (2 * kb + 2 * L) * G * h > N) continue;
      // short residue classes: the pipeline's fill (2 / 4 steps per chunk) is not amortised -- on sym8
      // 16384-sample signals through the tiled path a triple ran 21.2 ms vs 12.3 for pairs
      // (profiles/r03/ab_sweepg_short.log); such levels keep one sweep each
      if (N / h < (int64_t)tu.sweep2_minb * kb) continue;
      *ka_out = ka;
      *r_out = r;
      return true;
    }
  }
  return false;
}

// Streaming deep group (vw_deep.hip): PERIODIC levels jlo..jhi of the per-level path in one launch.
// Needs level jlo's spacing P to divide N and hold C = 64 bytes of residues; every ring of the group
// within the LDS budget.  Ring capacities: DMA-fed rings hold their history + two tiles (the next
// tile lands while the current one computes), multiples of 16 positions (one wave's DMA);
// level-fed rings history + one tile.  Returns the LDS bytes, 0 if the group does not qualify.
constexpr int kDeepTile = 128;  // vw_deep.hip kDeepT

template <typename T>
static int deep_plan(const Tuning& tu, const LevelDesc* lv, int jlo, int jhi, int L, int64_t N, bool inverse,
                     DeepArgs<T>* a) {
  const int C = 64 / (int)sizeof(T);
  const int g = jhi - jlo + 1;
  if (!(inverse ? tu.deep_inv : tu.deep) || g < 1 || g > kMaxGroup || !has_unrolled_taps(L)) return 0;
  const int P = lv[jlo - 1].s;
  if (P < C || P % C != 0 || N % P != 0 || N / P < 2 * kDeepTile) return 0;
  for (int j = jlo; j <= jhi; ++j)
    if (lv[j - 1].mode != kHaloPeriodic) return 0;
  int caps[2 * kMaxGroup] = {}, nr = 0;
  int64_t reach = 0;
  const int D = inverse ? tu.deep_pf_inv : tu.deep_pf_fwd;
  for (int k = 0; k < g; ++k) {
    const int64_t H = (int64_t)(L - 1) << k;
    reach += H;
    const bool dma_fed = inverse ? (k == g - 1) : (k == 0);
    caps[k] = dma_fed ? (int)round_up(H + (D + 1) * kDeepTile, 16) : (int)(H + kDeepTile);
    if (inverse) caps[g + k] = (int)round_up(H + (D + 1) * kDeepTile, 16);
  }
  nr = inverse ? 2 * g : g;
  int64_t pos = 0;
  for (int r = 0; r < nr; ++r) pos += caps[r];
  const int64_t bytes = pos * 64;
  if (bytes > (int64_t)tu.deep_lds * 1024 || bytes > kLdsBytes) return 0;
  if (a) {
    a->P = P; a->C = C; a->nq = (int)(N / P); a->nb = P / C; a->g = g; a->N = (int)N;
    a->warm = (int)round_up(reach, kDeepTile);
    a->depth = D;
    int64_t o = 0;
    for (int r = 0; r < nr; ++r) { a->cap[r] = caps[r]; a->off[r] = (int)(o * C); o += caps[r]; }
  }
  return (int)bytes;
}

// Segments per residue block: enough workgroups for `deep_waves` per CU, each segment at least four
// warm-ups long (the warm-up is recomputed per segment).
template <typename T>
static void deep_segments(const Tuning& tu, int cus, int64_t B, DeepArgs<T>* a) {
  const int64_t wg0 = B * a->nb;
  int64_t seg = std::max<int64_t>(1, ((int64_t)tu.deep_waves * cus + wg0 - 1) / wg0);
  seg = std::min<int64_t>(seg, std::max<int64_t>(1, a->nq / (4 * (int64_t)a->warm)));
  a->seg = (int)seg;
  a->seglen = (int)round_up((a->nq + seg - 1) / seg, kDeepTile);
  a->seg = (int)((a->nq + a->seglen - 1) / a->seglen);
}

template <typename T>
static PlanStep<T>& add_step(std::vector<PlanStep<T>>& steps, int kind, int jlo, int jhi, int src, int dst) {
  steps.emplace_back();
  PlanStep<T>& s = steps.back();
  memset(static_cast<void*>(&s), 0, sizeof(s));
  s.kind = kind; s.jlo = jlo; s.jhi = jhi; s.src = src; s.dst = dst;
  return s;
}

// The fix-up after the launches (vw_ref.hip): rows recomputed at once, one workgroup each with two
// running-approximation rows of scratch (<= 512 MiB), and the row flags.
template <typename T, typename P>
static void reserve_ref(const Tuning& tu, int cus, int64_t B, int64_t N, P* p) {
  if (!p->ref_nf) return;
  int64_t grid = std::min<int64_t>(B, tu.ref_grid > 0 ? tu.ref_grid : 2LL * cus);
  grid = std::max<int64_t>(1, std::min<int64_t>(grid, ((int64_t)512 << 20) / (2 * N * (int64_t)sizeof(T))));
  p->res.ref_grid = (int)grid;
  p->res.nf_rows = B;
  p->res.ws_bytes = std::max(p->res.ws_bytes, (size_t)grid * 2 * (size_t)N * sizeof(T));
}

// ------------------------------------------------------------------------------------------------
// Forward (multi-level and single-level share this path).

// Level descriptors of the forward; returns the longest left halo.  c.L is the kernels' tap count (the longer
// filter of a two-length bank); Llo / Lhi the filters' own lengths (0 = c.L), which decide the FFT-switch mode:
// the outer gate reads the low-pass length, behind it each filter takes the FFT branch by its own length.
// *mixed = the first level where exactly one of them does (0 = none).
template <typename T>
static int forward_levels(const FwdCall<T>& c, LevelDesc* lv, int Llo = 0, int Lhi = 0, int* mixed = nullptr) {
  int max_hl = 0;
  if (Llo <= 0) Llo = c.L;
  if (Lhi <= 0) Lhi = c.L;
  for (int j = 1; j <= c.J; ++j) {
    LevelDesc& d = lv[j - 1];
    memset(&d, 0, sizeof(d));
    d.s = 1 << (j - 1);
    const int64_t Lj = upsampled_length(c.L, j);
    d.hl = (int)(Lj - 1);
    d.hr = 0;
    d.hist_len = (int)(Lj - 1);
    if (c.boundary == VW_PERIODIC) {
      d.mode = kHaloPeriodic;
      // MultiLevelMODWTTransform.applyScaledMODWT :734-742 + WaveletOperations :31-33 + FftHeuristics :30-34
      const int64_t Llo_j = upsampled_length(Llo, j), Lhi_j = upsampled_length(Lhi, j);
      if ((c.flags & VW_FLAG_FFT_SWITCH) && !c.single_level && !(c.N < 64 || Llo_j > c.N / 2) && c.N >= 1024 &&
          !is_pow2(c.N)) {
        const bool fft_lo = (double)Llo_j > c.N * (1.0 / 8.0), fft_hi = (double)Lhi_j > c.N * (1.0 / 8.0);
        if (fft_lo && fft_hi) d.mode = kHaloFftPad;
        else if (fft_lo != fft_hi && mixed && !*mixed) *mixed = j;
      }
    } else {
      d.mode = c.boundary == VW_ZERO_PADDING ? kHaloZero : kHaloSymmetric;
    }
    if (c.mode_override >= 0) d.mode = c.mode_override;
    max_hl = std::max(max_hl, d.hl);
  }
  return max_hl;
}

// Fused forward: one launch for all levels.  Returns false when the signal does not fit (per-level path).
//
// Level buffers: two (one barrier per level) or one (two barriers per level, but half the LDS:
// twice the workgroups per CU).  Measured on MI355X (db4 J=6, 4096 x 4096 fp64): two buffers win
// whenever the persistent forward (which needs them) runs -- FMA and EXACT alike; without it the
// EXACT kernel is faster with one buffer (more workgroups to overlap its longer arithmetic).
// VW_FWD_BUF=1|2 overrides.
//
// Persistent variant (vw_dev_fwd.h k_forward_persist): next row by LDS-DMA during the last level.
// Its contract: two buffers, full slabs of whole waves, rows in 64-vector chunks, no validation
// or streaming history.  VW_FWD_PERSIST=0 disables it.
template <typename T>
static bool plan_forward_fused(const Tuning& tu, const FwdCall<T>& c, int max_hl, FwdPlan<T>* p, bool bi = false) {
  constexpr int V = vec_width<T>();
  const int64_t N = c.N, nvec = (N + V - 1) / V;
  const int L = c.L, J = c.J;
  const bool validate = p->validate, hist = c.hist != nullptr;
  FwdArgs<T>& a = p->args;
  const int hlpad = (int)round_up(max_hl, V);
  const bool io_aligned =
      (c.ldx % V == 0) && (N % V == 0) && aligned16(c.x) && aligned16(c.details) && aligned16(c.approx);
  int threads = 0, lds = 0, nv = 4;
  auto persist_ok = [&](int th, int nvv, bool ft) {
    return !bi && tu.fwd_persist && io_aligned && ft && nvv == 4 && !validate && !hist && (int64_t)th * nvv == nvec &&
           th % 64 == 0 && nvec % 64 == 0 && has_unrolled_taps(L) && J >= 1;
  };
  const int64_t region = round_up(hlpad + nvec * V + V, V);
  bool dbl = tu.fwd_buf ? tu.fwd_buf == 2 : true;
  bool fused = false, fit = false;
  // NV = 2 (1024-thread workgroups) only where the unrolled kernel will run (it has no runtime-L form)
  const int fwd_nv2 = (!bi && tu.fwd_nv == 2 && io_aligned && L <= 8 && L <= tu.unroll_max && has_unrolled_taps(L) &&
                       !(tu.blk > 0 && L >= tu.blk)) ? 2 : 0;
  if (J <= kMaxLevels && !tu.force_tiled) {
    if (dbl) dbl = fused_plan(tu, N, V, sizeof(T), 2 * region, &threads, &nv, &lds, &fit, fwd_nv2);
    if (dbl && !tu.fwd_buf && !p->fma && !persist_ok(threads, nv, fit)) dbl = false;  // EXACT without persistence
    fused = dbl || fused_plan(tu, N, V, sizeof(T), region, &threads, &nv, &lds, &fit, fwd_nv2);
  }
  if (!fused) return false;
  if (nv == 2 && !(fit && (int64_t)threads * 2 == nvec)) {
    plan_error(p, VW_ERR_STATE, "NV=2 plan without full slabs");
    return true;
  }
  for (int j = 0; j < J; ++j) set_halo_images(a.lv[j], N, a.npow2, V, threads, nv);
  a.hlpad = hlpad; a.region1 = dbl ? (int)region : 0;
  a.vec_io = io_aligned;
  a.unrolled = a.vec_io && fit && L <= tu.unroll_max;
  a.rev = tu.fwd_rev;
  a.level_ct = tu.level_ct;
  // non-temporal LDS-DMA of the rows: faster at <= 2 signals per CU (512 rows: forward 0.0268 -> 0.0245 ms),
  // slower on full batches (4096 rows: 0.218-0.225 -> 0.234-0.243 ms; profiles/r04/ab_rotate_default_*.log,
  // ab_overlap_direct_512.log)
  a.dma_nt = tu.dma_nt >= 0 ? tu.dma_nt : (c.B <= 2LL * c.cus ? 1 : 0);
  p->kernel = (dbl && a.unrolled && persist_ok(threads, nv, fit)) ? kFwdPersist : kFwdFused;
  // register-blocked PERIODIC forward for long filters (vw_blk.h k_forward_blk): padded layouts
  // (NV = 8, 1024-thread workgroups: with its taps from the kernel arguments (round 4, 99 VGPRs, no
  // spills) the blocked forward beats the fused one at sym8 N = 16384: 5.27-5.29 -> 4.76 ms,
  // profiles/r04/ab_blk_fwd8_ktaps_sym8.log; VW_BLK_FWD8=0 restores the fused kernel)
  // (listed tap counts only: launch_forward_blk has no runtime-L form)
  if (!bi && tu.blk > 0 && L >= tu.blk && has_unrolled_taps(L) && a.unrolled && !validate && !hist &&
      (int64_t)threads * nv == nvec && (nv == 4 || (nv == 8 && tu.blk_fwd8))) {
    const BlkPlan b = blk_plan<T>(a.lv, J, L, nvec, nv, false);
    a.blk_tight = b.tight;
    if (b.ok) {
      const bool two = 2 * b.buf * 16 <= 80 * 1024;  // two buffers only where two workgroups still fit a CU
      a.region1 = two ? (int)(b.buf * V) : 0;
      a.hlpad = b.hlv * V;
      a.tap_lds = (int)(b.buf * V * (two ? 2 : 1));
      const int blk_lds = (int)(b.buf * 16 * (two ? 2 : 1)) + 2 * L * (int)sizeof(T);
      if (blk_lds <= kLdsBytes) {
        lds = blk_lds;
        p->kernel = kFwdBlk;
      }
    }
  }
  // fp32 FMA, PERIODIC, long filters: the matrix-core forward (vw_mfma.hip, VW_MFMA bit 0)
  if (std::is_same<T, float>::value) {
    bool ok = !bi && (tu.mfma & 1) && p->fma && !c.single_level && a.vec_io && !validate && !hist;
    for (int j = 0; ok && j < J; ++j) ok = a.lv[j].mode == kHaloPeriodic;
    const int scratch = 8 * 256 + 4;  // the forward's per-wave transpose scratch (<= 8 waves), aligned
    if (const int mfma_lds = mfma_layout(ok, L, J, N, scratch, &a.hlpad, &a.tap_lds)) {
      lds = mfma_lds;
      p->kernel = kFwdMfma;
    }
  }
  // VW_FLAG_REF_NONFINITE: the persistent and the register-blocked forward probe their a_J (no scan pass
  // afterwards)
  p->nf_probed = p->ref_nf && (p->kernel == kFwdBlk || p->kernel == kFwdPersist);
  p->threads = threads; p->nv = nv; p->lds = lds;
  return true;
}

// Per-level path for long signals: ping-pong the running approximation through the workspace.
// Deep levels (s >= kSweepMinS) run as column sweeps, shallow ones as LDS tiles with a halo.
template <typename T>
static void plan_forward_levels(const Tuning& tu, const FwdCall<T>& c, FwdPlan<T>* p) {
  constexpr int V = vec_width<T>();
  const int64_t N = c.N;
  const int L = c.L, J = c.J;
  const bool validate = p->validate, hist = c.hist != nullptr;
  const LevelDesc* lv = p->args.lv;
  for (int j = 1; hist && j <= J; ++j)
    if (lv[j - 1].hist_len > N)
      return plan_error(p, VW_ERR_UNSUPPORTED, "streaming block shorter than level %d history", j);
  const int tile_max = tu.fwd_tile ? tu.fwd_tile / V * V : 256 * kNV * V;
  const size_t plane = (size_t)c.B * (size_t)N;
  p->res.ws_bytes = 2 * plane * sizeof(T) + 256;
  const StepAlign al{c.x, c.approx, c.details, plane * sizeof(T)};
  const int mtile = multi_tile<T>(tu);
  int groups[kMaxLevels];
  level_groups(tu, lv, J, L, V, mtile, !validate && !hist, groups);
  int src = kBufIn;
  int64_t lda = c.ldx;
  for (int j = 1; j <= J; ++j) {
    const int nxt = src == kBufWs0 ? kBufWs1 : kBufWs0;  // never the level's own input
    // streaming deep group from level j: the longest run j..je within the LDS budget
    if (groups[j - 1] == 1 && !validate && !hist && (lda % V) == 0 && al.buf(src) && aligned16(c.details) &&
        aligned16(c.approx) && deep_plan<T>(tu, lv, j, j, L, N, false, nullptr)) {
      int je = j;
      while (je < J && groups[je] == 1 && deep_plan<T>(tu, lv, j, je + 1, L, N, false, nullptr)) ++je;
      PlanStep<T>& s = add_step(p->steps, kStepDeep, j, je, src, je == J ? kBufOut : nxt);
      s.lds = deep_plan<T>(tu, lv, j, je, L, N, false, &s.deep);
      deep_segments<T>(tu, c.cus, c.B, &s.deep);
      s.deep.lda = lda; s.deep.B = c.B; s.deep.taps = L;
      s.probe = p->ref_nf && je == J;  // the deep launch writes a_J: it probes it (VW_FLAG_REF_NONFINITE)
      src = s.dst;
      lda = N;
      j = je;
      continue;
    }
    if (groups[j - 1] >= 2) {
      const int g = groups[j - 1], je = j + g - 1;
      PlanStep<T>& s = add_step(p->steps, kStepMulti, j, je, src, je == J ? kBufOut : nxt);
      MultiArgs<T>& m = s.multi;
      m.lda = lda;
      bool io = al.buf(src) && al.buf(s.dst);
      for (int k = 0; k < g; ++k) io = io && al.plane(j - 1 + k);
      m.ext[g] = 0;
      for (int k = g - 1; k >= 0; --k)
        m.ext[k] = m.ext[k + 1] + (int)round_up((int64_t)(L - 1) * lv[j - 1 + k].s, V);
      m.B = c.B; m.N = (int)N; m.tile = mtile; m.nlev = g; m.s0 = lv[j - 1].s;
      m.region = (int)round_up(m.ext[0] + mtile + V, V);
      m.vec_io = (N % V == 0) && (lda % V == 0) && io;
      m.taps = L;
      s.lds = (int)(2 * m.region * sizeof(T));
      src = s.dst;
      lda = N;
      j = je;
      continue;
    }
    const bool sweep = lv[j - 1].s >= kSweepMinS && has_unrolled_taps(L) && !tu.no_sweep;
    PlanStep<T>& s = add_step(p->steps, sweep ? kStepSweep : kStepTile, j, j, src, j == J ? kBufOut : nxt);
    LevelArgs<T>& a = s.lvl;
    a.lv = lv[j - 1];
    const int hp = (int)round_up(a.lv.hl, V);
    // deep levels have long halos: shrink the tile so tile + halo fits LDS
    const int64_t fit = ((int64_t)kLdsBytes / (int64_t)sizeof(T) - hp - 2 * V) / V * V;
    const int tile = (int)std::min<int64_t>(tile_max, fit);
    if (tile < 64 * V) return plan_error(p, VW_ERR_UNSUPPORTED, "level %d halo (%d samples) exceeds LDS", j, a.lv.hl);
    a.lda = lda;
    a.B = c.B; a.N = (int)N; a.tile = sweep ? tu.sweep_qc : tile; a.hlpad = hp;
    a.vec_io = (N % V == 0) && (lda % V == 0) && al.buf(src) && al.buf(s.dst) && al.plane(j - 1);
    a.validate = validate; a.npow2 = p->args.npow2; a.taps = L;
    s.lds = sweep ? 0 : (int)((hp + tile + V) * sizeof(T));
    // streaming: this level's new left history = the last L_j - 1 samples of its input
    // (BatchStreamingMODWT.updateHistoryFromSoA :337-352); read by this level's kernel first
    s.hist_update = hist && c.hist_update;
    src = s.dst;
    lda = N;
  }
  p->nf_probed = !p->steps.empty() && p->steps.back().probe;
}

template <typename C>
static int hi_taps(const C& c) { return c.Lhi > 0 ? c.Lhi : c.L; }

// Tap count the kernels run for a bank whose longer filter has `L` taps.  Most biorthogonal lengths are odd and
// none of those is in VW_TAP_LIST, so max(Llo, Lhi) would run the runtime-L kernels; one more zero tap reaches a
// listed count and with it the tap-unrolled, persistent, register-blocked, deep and sweep kernels (VW_BI_LISTED).
// The extra tap changes no bit (as every padded tap) and only lengthens the halos, which every path below sizes
// from the tap count it is given; a plan that fails with it is planned again without (plan_forward / plan_inverse).
static int listed_taps(const Tuning& tu, int L, bool two_lengths) {
  return (two_lengths && tu.bi_listed && !has_unrolled_taps(L) && L < kMaxTaps && has_unrolled_taps(L + 1)) ? L + 1 : L;
}

template <typename T>
static void plan_forward_taps(const Tuning& tu, const FwdCall<T>& call, int taps, FwdPlan<T>* p, bool bi = false) {
  // two lengths: the padded route (vw_plan.h) -- every kernel below sees one tap count
  FwdCall<T> c = call;
  const int Llo = call.L, Lhi = hi_taps(call);
  c.L = taps;
  c.Lhi = 0;
  const bool hist = c.hist != nullptr;
  p->fma = c.flags & VW_FLAG_FMA;
  p->validate = c.flags & VW_FLAG_VALIDATE;
  FwdArgs<T>& a = p->args;
  a.B = c.B; a.N = (int)c.N; a.J = c.J; a.ldx = c.ldx;
  a.npow2 = next_pow2(c.N);
  a.validate = p->validate;
  a.hist_update = c.hist_update ? 1 : 0;
  a.taps = c.L; a.taps_hi = c.L;
  int mixed = 0;
  const int max_hl = forward_levels(c, a.lv, Llo, Lhi, &mixed);
  if (mixed)
    return plan_error(p, VW_ERR_UNSUPPORTED, "FFT switch: one filter of level %d is in the FFT region, one is not (mixed level)",
                      mixed);
  // VW_FLAG_REF_NONFINITE on a streaming block: keep the histories this block reads (the kernels
  // overwrite them) for the rows vw_ref.hip recomputes
  p->snapshot = (c.flags & VW_FLAG_REF_NONFINITE) && hist && c.hist_update && c.hist_snap && !c.hist_first && c.J >= 2;
  // the unvalidated callers' NaN spread through the zero taps (single level and J = 1 have none); a
  // streaming block that updates its history needs the snapshot of the histories it read (stream_run)
  // A zero-extended filter has zero taps at level 1 too, where the reference's loops read nothing: there the
  // fix-up also covers J = 1 and the single-level forward.
  const bool padded = taps != Llo || taps != Lhi;
  p->ref_nf = (c.flags & VW_FLAG_REF_NONFINITE) && !p->validate && (padded || (!c.single_level && c.J >= 2)) &&
              !(c.flags & VW_FLAG_FFT_SWITCH) && (!hist || !c.hist_update || c.hist_first || c.hist_snap);
  p->fused = plan_forward_fused(tu, c, max_hl, p, bi);
  // the two-length route: planned for the longer reach, run at each filter's own count (unrolled only for a listed pair)
  // -- and by default only there: the runtime-L bodies lose to the padded route's unrolled kernels (VW_BI bit 2)
  if (bi && p->fused && !hist && p->nv != 2 && p->kernel == kFwdFused &&
      ((tu.bi & 4) || (a.unrolled && has_unrolled_pair(Llo, Lhi)))) {
    a.taps = Llo; a.taps_hi = Lhi;
    a.unrolled = a.unrolled && has_unrolled_pair(Llo, Lhi);
  }
  if (!p->fused) plan_forward_levels(tu, c, p);
  reserve_ref<T>(tu, c.cus, c.B, c.N, p);
}

// ------------------------------------------------------------------------------------------------
// Energy per level (vw_energy.hip).  The fused kernel is the VW_FLAG_TREE_SUMS path: it runs where the plain
// fused forward would -- the cascade fits LDS and 1024 threads x NV, any L and boundary -- but not for the
// calls whose forward does more than the cascade (validation, the FFT-switch levels, the REF_NONFINITE
// fix-up): those, and the default sequential sums, go through the forward's own plan and the plane sums.
// Level buffers, after the forward's measurements on the same cascade (plan_forward_fused): the EXACT arithmetic
// runs with one buffer (half the LDS, twice the workgroups to overlap its longer chains), FMA with two (one
// barrier per level) while two workgroups still fit a CU.  Whole waves
// (the kernel folds partials with wave butterflies); kEnergyRed doubles of wave partials follow the buffers.
void plan_energy(const Tuning& tu, const FwdCall<double>& c, EnergyPlan* p) {
  constexpr int V = vec_width<double>();
  const int64_t N = c.N, nvec = (N + V - 1) / V;
  const int L = c.L, J = c.J;
  EnergyArgs& a = p->args;
  p->fma = c.flags & VW_FLAG_FMA;
  p->fused = false;
  if (!(c.flags & VW_FLAG_TREE_SUMS) || tu.energy_fused == 0 || tu.force_tiled || J < 1 || J > kMaxLevels ||
      (c.flags & (VW_FLAG_VALIDATE | VW_FLAG_REF_NONFINITE)) || c.hist || c.single_level)
    return;
  const int max_hl = forward_levels(c, a.lv);
  for (int j = 0; j < J; ++j)
    if (a.lv[j].mode == kHaloFftPad) return;
  const int hlpad = (int)round_up(max_hl, V);
  const int64_t region = round_up(hlpad + nvec * V + V, V);
  int threads = 0, lds = 0, nv = 4;
  bool fit = false;
  bool dbl = p->fma && (2 * region + kEnergyRed) * (int64_t)sizeof(double) <= kLdsBytes / 2 &&
             fused_plan(tu, N, V, sizeof(double), 2 * region + kEnergyRed, &threads, &nv, &lds, &fit);
  if (!dbl && !fused_plan(tu, N, V, sizeof(double), region + kEnergyRed, &threads, &nv, &lds, &fit)) return;
  threads = (int)round_up(threads, 64);  // <= 512 (NV = 4) / 1024 (NV = 8): fused_plan's bounds are multiples of 64
  fit = (int64_t)(nv - 1) * threads <= nvec;
  const bool io_aligned = (c.ldx % V == 0) && (N % V == 0) && aligned16(c.x);
  a.B = c.B; a.N = (int)N; a.J = J; a.ldx = c.ldx;
  a.npow2 = next_pow2(N);
  a.taps = L;
  for (int j = 0; j < J; ++j) set_halo_images(a.lv[j], N, a.npow2, V, threads, nv);
  a.hlpad = hlpad;
  a.region1 = dbl ? (int)region : 0;
  a.red_off = (int)((dbl ? 2 : 1) * region);
  a.vec_io = io_aligned;
  a.unrolled = io_aligned && fit && L <= tu.unroll_max && L <= kEnergyUnrollMax && has_unrolled_taps(L);
  a.level_ct = tu.level_ct;
  // a few workgroups per CU, grid-stride over the rows: what LDS and the kernels' wave bounds
  // (k_energy_fused: 6 waves per SIMD for NV = 4 and L <= 8, else 4) let be resident at once
  const int wpe = (nv <= 4 && L <= 8) ? 6 : 4;
  const int by_waves = std::max(1, wpe * 4 / (threads / 64));
  const int by_lds = std::max(1, kLdsBytes / std::max(lds, 1));
  p->grid = (int)std::min<int64_t>(c.B, (int64_t)std::max(c.cus, 1) * std::min(by_waves, by_lds));
  p->threads = threads; p->nv = nv; p->lds = lds;
  p->fused = true;
}

// ------------------------------------------------------------------------------------------------
// Inverse

// Level descriptors of the inverse; the longest halos come back through max_hl / max_hr.
// c.L is the kernels' tap count, which bounds the reach of both branches; Llo / Lhi are the reconstruction
// filters' own lengths: decide() keys on the low-pass one, each branch shifts by its own tau (:604-608).
template <typename T>
static void inverse_levels(const InvCall<T>& c, int Llo, int Lhi, LevelDesc* lv, int* max_hl, int* max_hr) {
  constexpr int V = vec_width<T>();
  const int tmax = (int)((c.N + V - 1) / V * V - 1);
  for (int j = 1; j <= c.J; ++j) {
    LevelDesc& d = lv[j - 1];
    memset(&d, 0, sizeof(d));
    d.s = 1 << (j - 1);
    d.use_d = (c.detail_mask >> (j - 1)) & 1u;
    d.mode = ref_mode(c.boundary);
    if (c.boundary == VW_SYMMETRIC && !c.single_level) {
      int ap, dh, dp, dg;
      sym_decide(c.wid, Llo, j, &ap, &dh, &dp, &dg);
      const int tauH = compute_tau(Llo, j) + dh;
      const int tauG = compute_tau(Lhi, j) + dg;
      d.dir_a = ap ? 1 : -1; d.off_a = ap ? -tauH : tauH;
      d.dir_d = dp ? 1 : -1; d.off_d = dp ? -tauG : tauG;
    } else if (c.boundary == VW_SYMMETRIC) {
      const int dir = (c.flags & VW_FLAG_BATCH_SYM_INVERSE) ? 1 : -1;  // inverseBatchOptimized (t+l) vs inverse (t-l)
      d.dir_a = d.dir_d = dir; d.off_a = d.off_d = 0;
    } else {
      d.dir_a = d.dir_d = 1; d.off_a = d.off_d = 0;
    }
    int hl = 0, hr = 0;
    branch_extent((int)c.N, tmax, c.L, d.s, d.dir_a, d.off_a, &hl, &hr);
    branch_extent((int)c.N, tmax, c.L, d.s, d.dir_d, d.off_d, &hl, &hr);
    d.hl = hl; d.hr = hr;
    *max_hl = std::max(*max_hl, hl);
    *max_hr = std::max(*max_hr, hr);
  }
}

// The PLAIN class of inverse calls (vw_dev_inv.h inverse_seq_plain): a full-slab fp64 PERIODIC reconstruction of a short
// filter from every coefficient plane, forward walk, no threshold, no probe -- every level reads t + i*s with no
// left halo and a right one within the row.  Independent of the LDS buffer count: plan_inverse_fused marks
// k_inverse_seq plans of the class (InvArgs::plain), pair_fusable also takes k_inverse_db plans of it.  Reads
// a.full / a.rev / a.lv and p.ref_nf: call once those are set.
template <typename T>
static bool plain_class(const InvCall<T>& c, const InvPlan<T>& p, int nv) {
  const InvArgs<T>& a = p.args;
  if (!(a.full && sizeof(T) == 8 && nv == 4 && c.L <= 8 && c.boundary == VW_PERIODIC && !c.thr && !c.approx_zero &&
        !a.rev && !p.ref_nf))
    return false;
  for (int j = 0; j < c.J; ++j)
    if (!(a.lv[j].use_d && plus_zero(a.lv[j]) && a.lv[j].hl == 0 && a.lv[j].hr <= c.N)) return false;
  return true;
}

// Fused inverse: one launch for all levels.  Returns false when the signal does not fit (per-level path).
//
// Pairwise sums need a_j and d_j together (two regions).  Sequential sums time-share one region
// (k_inverse_seq, four barriers per level) -- measured faster on MI355X than two buffers
// (k_inverse_db, two barriers per level) because twice the workgroups fit per CU; VW_INV_BUF=2
// selects the latter.
// Two LDS buffers (two barriers per level, two workgroups per CU) vs one (four barriers, three per
// CU): with at most 2 signals per CU the occupancy of the one-buffer kernel is not reached and the
// shorter per-level chain wins (measured on MI355X, db4 x 4096, inverse ms one / two buffers:
// B = 512 0.0335 / 0.0324, B = 768 0.0462 / 0.0504, B = 1024 0.0594 / 0.0606 --
// profiles/r02/ab_small_batch.log, ab_inv_buf_1024_768.log); VW_INV_BUF=1|2 overrides.
// Long PERIODIC filters (L >= VW_BLK) keep the register-blocked single-buffer kernel (k_inverse_blk
// needs !db) at small batches too: its NV+L-1 LDS reads per branch outweigh the shorter barrier chain.
// Only listed tap counts have a k_inverse_blk: other lengths follow the short filters' policy.
// (A persistent form that loads the next signal's approximation during level 1 was measured
// slower on MI355X: 3 resident workgroups per CU do not divide the batch evenly, and the dynamic
// dispatch of one-signal workgroups balances better.)
template <typename T>
static bool plan_inverse_fused(const Tuning& tu, const InvCall<T>& c, bool pair, int max_hl, int max_hr,
                               InvPlan<T>* p, bool bi = false) {
  constexpr int V = vec_width<T>();
  const int64_t N = c.N, nvec = (N + V - 1) / V;
  const int L = c.L, J = c.J;
  const bool periodic = c.boundary == VW_PERIODIC;
  InvArgs<T>& a = p->args;
  const int hlpad = (int)round_up(max_hl, V);
  const int64_t region = round_up(hlpad + nvec * V + max_hr + V, V);
  int threads = 0, lds = 0, nv = 4;
  // bi: the two-length route keeps to k_inverse_seq / k_inverse_db (no register-blocked or matrix-core form)
  const bool blk_pref = !bi && tu.blk > 0 && L >= tu.blk && has_unrolled_taps(L) && periodic;
  bool db = !pair && (tu.inv_buf ? tu.inv_buf == 2 : (c.B <= 2LL * c.cus && !blk_pref));
  bool fused = false, fit = false;
  const bool inv_io = (N % V == 0) && aligned16(c.details) && aligned16(c.approx) && aligned16(c.y);
  const int inv_nv2 = (tu.inv_nv == 2 && inv_io && L <= 8 && L <= tu.unroll_max && has_unrolled_taps(L)) ? 2 : 0;
  if (!tu.force_tiled) {
    if (pair || db) fused = fused_plan(tu, N, V, sizeof(T), 2 * region, &threads, &nv, &lds, &fit, inv_nv2);
    if (!fused && !pair) {
      db = false;
      fused = fused_plan(tu, N, V, sizeof(T), region, &threads, &nv, &lds, &fit, inv_nv2);
    }
  }
  if (!fused) return false;
  for (int j = 0; j < J; ++j) set_halo_images(a.lv[j], N, 0, V, threads, nv);
  a.db = db ? 1 : 0;
  a.hlpad_a = hlpad; a.hlpad_d = hlpad; a.region_d = (int)region;
  a.vec_io = inv_io;
  a.unrolled = a.vec_io && fit && L <= tu.unroll_max;
  a.pair = pair;
  a.rev = tu.inv_rev;
  a.level_ct = tu.level_ct;
  a.full = tu.level_ct && a.unrolled && (int64_t)threads * nv == nvec;
  p->kernel = pair ? kInvPair : db ? kInvDb : kInvSeq;
  // register-blocked PERIODIC inverse for long filters (vw_blk.h k_inverse_blk)
  if (!bi && tu.blk > 0 && L >= tu.blk && has_unrolled_taps(L) && nv != 2 && !pair && !db && periodic && a.unrolled &&
      (int64_t)threads * nv == nvec) {
    const BlkPlan b = blk_plan<T>(a.lv, J, L, nvec, nv, true);
    a.blk_tight = b.tight;
    if (b.ok) {
      a.blk = 1;
      a.tap_lds = (int)(b.buf * V);
      lds = (int)(b.buf * 16) + 2 * L * (int)sizeof(T);
      p->kernel = kInvBlk;
    }
  }
  // fp32 FMA, PERIODIC sequential sums, long filters: the matrix-core inverse (vw_mfma.hip, VW_MFMA bit 1)
  if (std::is_same<T, float>::value) {
    bool ok = !bi && (tu.mfma & 2) && p->fma && !pair && periodic && a.vec_io;
    for (int j = 0; ok && j < J; ++j) ok = plus_zero(a.lv[j]);
    if (const int mfma_lds = mfma_layout(ok, L, J, N, 0, &a.hlpad_a, &a.tap_lds)) {
      lds = mfma_lds;
      p->kernel = kInvMfma;
    }
  }
  // VW_FLAG_REF_NONFINITE: the one-buffer sequential kernels (k_inverse_seq / k_inverse_blk, vw_inv.hip's
  // choice) probe their output themselves (no scan pass afterwards)
  p->nf_probed = p->ref_nf && (p->kernel == kInvSeq || p->kernel == kInvBlk);
  // k_inverse_seq's PLAIN form (vw_dev_inv.h inverse_seq_plain; fp64 short filters, vw_inv.hip's dispatch): a
  // full-slab PERIODIC reconstruction that uses none of the general form's optional state
  a.plain = p->kernel == kInvSeq && plain_class(c, *p, nv) ? 1 : 0;
  a.waves = tu.inv_waves;
  p->threads = threads; p->nv = nv; p->lds = lds;
  return true;
}

// k_inverse_multi's layout for the group j0 .. j0+g-1 (m.ext filled): prefetch, padded regions, and
// four output vectors per thread (fp64, padded layouts): at NI = 8 a 2048-sample tile gives the
// register-blocked levels 129-144 threads of work, i.e. 2.0-2.3 of the workgroup's 4 waves (one SIMD idle,
// one mostly idle); at NI = 4 on the largest tile whose levels fit 256 threads (1792 for db8) all four
// waves work.  The group itself stays as level_groups planned it.
template <typename T>
static void inverse_multi_layout(const Tuning& tu, const LevelDesc* lv, int j0, int g, int L, int mtile,
                                 MultiArgs<T>& m) {
  constexpr int V = vec_width<T>();
  m.region = (int)round_up(mtile + m.ext[g - 1] + V, V);
  m.rblk = tu.multi_rblk;
  // register prefetch of d_{j-1} while level j computes: whole vectors, every tile of the group
  m.pf = tu.multi_pf && m.vec_io && (int64_t)(mtile + m.ext[g - 1]) / V <= (int64_t)kMultiPF * 256;
  // padded layout at the register-blocked levels (vw_dev_lvl.h k_inverse_multi): needs the register
  // paths (prefetch, blocked taps); the regions grow by one vector in eight
  m.pad = tu.multi_pad && m.pf && m.rblk && has_unrolled_taps(L);
  if (m.pad) {
    const int nvmax = (mtile + m.ext[g - 1]) / V + 1;
    m.region = (nvmax + nvmax / 8 + 1) * V;
  }
  // slack past D for the compile-time-stride reads (vw_dev_lvl.h k_inverse_multi): 15*M <= 120 vectors
  m.slack = 160;
  m.ni = kMultiInvNI;
  if (tu.multi_ni == 4 && sizeof(T) == 8 && m.pad) {
    auto fits = [&](int64_t t) {
      if ((t + m.ext[g - 1]) / V > (int64_t)kMultiPF * 256) return false;
      for (int k = 0; k < g; ++k) {
        const int64_t s = lv[j0 - 1 + k].s, M = s % V == 0 ? s / V : 0;
        const int64_t nv = (t + (k > 0 ? m.ext[k - 1] : 0)) / V;
        const bool blk = M == 1 || M == 2 || M == 4 || M == 8;
        if (blk ? (nv + 4 * M - 1) / (4 * M) * M > 256 : nv > 4 * 256) return false;
      }
      return true;
    };
    int64_t t = mtile;
    while (t >= 512 && !fits(t)) t -= 64 * V;
    if (t >= 512) {
      m.ni = 4;
      m.tile = (int)t;
      const int nvmax = (int)((t + m.ext[g - 1]) / V) + 1;
      m.region = (nvmax + nvmax / 4 + 1) * V;  // layouts 2 / 3 add at most u/4
    }
  }
}

// Per-level inverse, from level J down.
// 1024-sample tiles: two LDS regions of ~9 KiB keep many workgroups per CU (measured best on
// MI355X for db8 2^20-sample blocks; VW_INV_TILE overrides)
template <typename T>
static void plan_inverse_levels(const Tuning& tu, const InvCall<T>& c, bool pair, InvPlan<T>* p) {
  constexpr int V = vec_width<T>();
  const int64_t N = c.N;
  const int L = c.L, J = c.J;
  const bool periodic = c.boundary == VW_PERIODIC;
  const LevelDesc* lv = p->args.lv;
  const int tile_max = tu.inv_tile ? tu.inv_tile / V * V : 1024;
  const size_t plane = (size_t)c.B * (size_t)N;
  p->res.ws_bytes = 2 * plane * sizeof(T) + 256;
  const StepAlign al{c.approx, c.y, c.details, plane * sizeof(T)};
  auto plane_al = [&](int j) { return !lv[j - 1].use_d || al.plane(j - 1); };  // a masked level reads no plane
  // multi-level groups (PERIODIC sequential sums): start level of the group whose top is j
  const int mtile = tu.multi_inv_tile >= 64 * V ? tu.multi_inv_tile / V * V : multi_tile<T>(tu);
  int groups[kMaxLevels], start_of[kMaxLevels + 1] = {};
  level_groups(tu, lv, J, L, V, mtile, !pair && periodic, groups);
  for (int j = 1; j <= J; ++j) {
    if (groups[j - 1] < 2) continue;
    int64_t ext = 0;  // k_inverse_multi holds (tile + reach) / V vectors in kMultiInvNI per thread
    for (int k = 0; k < groups[j - 1]; ++k) ext += round_up((int64_t)(L - 1) * lv[j - 1 + k].s, V);
    if ((mtile + ext) / V <= (int64_t)kMultiInvNI * 256) start_of[j + groups[j - 1] - 1] = j;
  }
  char in_group[kMaxLevels + 1] = {};  // levels inside a multi-level tile group
  for (int e = 1; e <= J; ++e)
    for (int k = start_of[e]; start_of[e] > 0 && k <= e; ++k) in_group[k] = 1;
  int cur = c.approx_zero ? kBufNone : kBufIn;
  for (int j = J; j >= 1; --j) {
    const int nxt = cur == kBufWs0 ? kBufWs1 : kBufWs0;  // never the level's own input
    // streaming deep group with top level j: the lowest jl whose group jl..j fits the LDS budget
    if (!pair && periodic && !in_group[j] && al.buf(cur) && aligned16(c.details) && aligned16(c.y) &&
        deep_plan<T>(tu, lv, j, j, L, N, true, nullptr)) {
      int jl = j;
      while (jl > 1 && !in_group[jl - 1] && deep_plan<T>(tu, lv, jl - 1, j, L, N, true, nullptr)) --jl;
      PlanStep<T>& s = add_step(p->steps, kStepDeep, jl, j, cur, jl == 1 ? kBufOut : nxt);
      s.lds = deep_plan<T>(tu, lv, jl, j, L, N, true, &s.deep);
      deep_segments<T>(tu, c.cus, c.B, &s.deep);
      s.deep.lda = N; s.deep.B = c.B; s.deep.taps = L; s.deep.soft = c.soft;
      cur = s.dst;
      j = jl;
      continue;
    }
    if (start_of[j] > 0) {
      const int j0 = start_of[j], g = j - j0 + 1;
      PlanStep<T>& s = add_step(p->steps, kStepMulti, j0, j, cur, j0 == 1 ? kBufOut : nxt);
      MultiArgs<T>& m = s.multi;
      s.probe = p->ref_nf && j0 == 1;  // the group writes y: it probes it (VW_FLAG_REF_NONFINITE)
      bool io = al.buf(cur) && al.buf(s.dst);
      for (int k = 0; k < g; ++k) {
        io = io && plane_al(j0 + k);
        m.ext[k] = (k > 0 ? m.ext[k - 1] : 0) + (int)round_up((int64_t)(L - 1) * lv[j0 - 1 + k].s, V);
      }
      m.B = c.B; m.N = (int)N; m.tile = mtile; m.nlev = g; m.s0 = lv[j0 - 1].s;
      m.vec_io = (N % V == 0) && io;
      m.soft = c.soft; m.taps = L;
      inverse_multi_layout<T>(tu, lv, j0, g, L, mtile, m);
      s.lds = (int)((2 * m.region + m.slack * V) * sizeof(T));
      cur = s.dst;
      j = j0;
      continue;
    }
    // two or three column-sweep levels per launch (k_inverse_sweep2 / 3): the intermediate
    // approximations stay in LDS rings
    if (tu.sweep2 && !tu.deep_inv && !tu.no_sweep && !pair && j >= 2 && has_unrolled_taps(L)) {
      int G = 0, ka = 0, R = 0;
      for (int levels = std::min(tu.sweep2 >= 3 ? 3 : 2, j); levels >= 2 && !G; --levels)
        if (sweepg_plan<T>(tu, lv, j, levels, L, N, in_group, start_of, &ka, &R)) G = levels;
      if (G) {
        PlanStep<T>& s = add_step(p->steps, kStepSweepG, j - G + 1, j, cur, j == G ? kBufOut : nxt);
        LevelArgs<T>& a = s.lvl;
        a.lv = lv[j - 1];
        a.use_d = lv[j - 1].use_d;
        a.use_d2 = lv[j - 2].use_d;
        if (G == 3) a.use_d3 = lv[j - 3].use_d;
        a.soft = c.soft;
        a.B = c.B; a.N = (int)N; a.taps = L;
        s.G = G == 2 ? 2 : 4; s.ka = ka; s.R = R;
        a.tile = (int)round_up(tu.sweep2_uc, s.G * ka);
        cur = s.dst;
        j -= G - 1;  // levels j-1 (, j-2) done too
        continue;
      }
    }
    const bool sweep = lv[j - 1].s >= kSweepMinS && has_unrolled_taps(L) && !tu.no_sweep;
    PlanStep<T>& s = add_step(p->steps, sweep ? kStepSweep : kStepTile, j, j, cur, j == 1 ? kBufOut : nxt);
    LevelArgs<T>& a = s.lvl;
    a.lv = lv[j - 1];
    const int hp = (int)round_up(a.lv.hl, V);
    const int64_t fit = ((int64_t)kLdsBytes / (int64_t)sizeof(T) / 2 - hp - a.lv.hr - 2 * V) / V * V;
    const int tile = (int)std::min<int64_t>(tile_max, fit);
    if (tile < 64 * V) return plan_error(p, VW_ERR_UNSUPPORTED, "level %d halo exceeds LDS", j);
    const int64_t reg = round_up(hp + tile + a.lv.hr + V, V);
    a.use_d = a.lv.use_d;
    a.B = c.B; a.N = (int)N; a.tile = sweep ? tu.sweep_qc : tile; a.hlpad = hp; a.hlpad_d = hp; a.region_d = (int)reg;
    a.pair = pair; a.soft = c.soft; a.taps = L;
    a.vec_io = (N % V == 0) && al.buf(s.dst) && al.buf(cur) && plane_al(j);
    s.lds = sweep ? 0 : (int)(2 * reg * sizeof(T));
    cur = s.dst;
  }
  p->nf_probed = !p->steps.empty() && p->steps.back().probe;
}

// `taps`: the sequential sums' tap count (>= both lengths); the pairwise sums run the low-pass length
template <typename T>
static void plan_inverse_taps(const Tuning& tu, const InvCall<T>& call, int taps, InvPlan<T>* p, bool bi = false) {
  InvCall<T> c = call;
  const int Llo = call.L, Lhi = hi_taps(call);
  const bool pair = c.single_level || c.boundary == VW_ZERO_PADDING;
  // two lengths (vw_plan.h): the pairwise sums run over l < Llo and read high[l] (:591-601, MODWTTransform.inverse
  // :203-299) -- the longer high-pass truncated, a shorter one an ArrayIndexOutOfBoundsException in the reference;
  // the sequential sums take the padded route
  if (pair && Lhi < Llo)
    return plan_error(p, VW_ERR_UNSUPPORTED, "pairwise inverse: the reference indexes past its high-pass array (%d < %d taps)",
                      Lhi, Llo);
  c.L = pair ? Llo : taps;
  c.Lhi = 0;
  p->fma = c.flags & VW_FLAG_FMA;
  // the unvalidated callers' NaN spread through the zero taps (single level and J = 1 have none)
  // -- nor do the pairwise sums, whose longer high-pass is truncated; a zero-extended filter of the sequential
  // sums has zero taps at level 1 too, so there the fix-up also covers J = 1
  const bool padded = !pair && (c.L != Llo || c.L != Lhi);
  p->ref_nf = (c.flags & VW_FLAG_REF_NONFINITE) && (padded || (!c.single_level && c.J >= 2));
  InvArgs<T>& a = p->args;
  a.B = c.B; a.N = (int)c.N; a.J = c.J;
  a.approx_zero = c.approx_zero; a.thr_ld = c.thr_ld; a.soft = c.soft; a.taps = c.L; a.taps_hi = c.L;
  int max_hl = 0, max_hr = 0;
  inverse_levels(c, Llo, Lhi, a.lv, &max_hl, &max_hr);
  p->fused = plan_inverse_fused(tu, c, pair, max_hl, max_hr, p, bi);
  // the two-length route: planned for the longer reach, run at each branch's own count (unrolled only for a listed pair)
  // -- and by default only there: the runtime-L bodies lose to the padded route's unrolled kernels (VW_BI bit 2)
  if (bi && p->fused && !pair && p->nv != 2 && (p->kernel == kInvSeq || p->kernel == kInvDb) &&
      ((tu.bi & 4) || (a.unrolled && has_unrolled_pair(Llo, Lhi)))) {
    a.taps = Llo; a.taps_hi = Lhi;
    a.unrolled = a.unrolled && has_unrolled_pair(Llo, Lhi);
    a.full = 0;
    a.plain = 0;
  }
  if (!p->fused) plan_inverse_levels(tu, c, pair, p);
  reserve_ref<T>(tu, c.cus, c.B, c.N, p);
}

// ------------------------------------------------------------------------------------------------
// Multiresolution analysis (vw_mra.hip, vw_plan.h).  The level descriptors are inverse_levels' for the call with
// every plane kept, so each level's halos cover both branches' reach and the SYMMETRIC orientation and tau of
// each branch are the inverse's own.  Two regions, always (the ping-pong is what makes a pass one barrier);
// whole waves, as plan_energy.
template <typename T>
void plan_mra(const Tuning& tu, const InvCall<T>& c, MraPlan<T>* p) {
  constexpr int V = vec_width<T>();
  const int64_t N = c.N, nvec = (N + V - 1) / V;
  const int L = c.L, J = c.J;
  MraArgs<T>& a = p->args;
  p->fma = c.flags & VW_FLAG_FMA;
  p->fused = false;
  if (tu.mra_fused == 0 || tu.force_tiled || c.single_level || J < 1 || J > kMaxLevels || L < 1 || L > kMaxTaps ||
      (c.flags & (VW_FLAG_VALIDATE | VW_FLAG_REF_NONFINITE)) || (c.Lhi != 0 && c.Lhi != L) || c.thr)
    return;
  InvCall<T> k = c;
  k.detail_mask = ~0u;
  k.approx_zero = 0;
  int max_hl = 0, max_hr = 0;
  inverse_levels(k, L, L, a.lv, &max_hl, &max_hr);
  const int64_t hlpad = round_up(max_hl, V);
  const int64_t region = round_up(hlpad + nvec * V + max_hr + V, V);
  int threads = 0, lds = 0, nv = 4;
  bool fit = false;
  if (!fused_plan(tu, N, V, sizeof(T), 2 * region, &threads, &nv, &lds, &fit)) return;
  threads = (int)round_up(threads, 64);  // <= 512 (NV = 4) / 1024 (NV = 8): fused_plan's bounds are multiples of 64
  fit = (int64_t)(nv - 1) * threads <= nvec;
  const bool io_aligned = (N % V == 0) && aligned16(c.details) && aligned16(c.approx) && aligned16(c.y);
  a.B = c.B; a.N = (int)N; a.J = J;
  a.taps = L;
  for (int j = 0; j < J; ++j) set_halo_images(a.lv[j], N, 0, V, threads, nv);
  a.hlpad = (int)hlpad;
  a.region1 = (int)region;
  a.vec_io = io_aligned;
  a.unrolled = io_aligned && fit && L <= tu.unroll_max && L <= kMraUnrollMax && has_unrolled_taps(L);
  a.level_ct = tu.level_ct;
  // "On only where no slower" (DESIGN.md 8j): where the masked inverses run their tap-unrolled kernels and k_mra
  // has only its runtime-L body -- listed lengths past kMraUnrollMax on aligned full-slab rows -- the loop wins
  // (coif5 fp32 16384 x 8192, J = 6: 14.3 ms against 22.9 ms); VW_MRA_FUSED=2 fuses there too.
  if (tu.mra_fused == 1 && !a.unrolled && io_aligned && fit && L <= tu.unroll_max && has_unrolled_taps(L)) return;
  // a few workgroups per CU, grid-stride over the rows: what LDS and the kernel's wave bounds (k_mra: 6 waves per
  // SIMD at NV = 4 unless a long filter's unrolled body runs, else 4) let be resident at once
  const int wpe = (nv <= 4 && !(a.unrolled && L > 8)) ? 6 : 4;
  const int by_waves = std::max(1, wpe * 4 / (threads / 64));
  const int by_lds = std::max(1, kLdsBytes / std::max(lds, 1));
  p->grid = (int)std::min<int64_t>(c.B, (int64_t)std::max(c.cus, 1) * std::min(by_waves, by_lds));
  p->threads = threads; p->nv = nv; p->lds = lds;
  p->fused = true;
}
template void plan_mra<float>(const Tuning&, const InvCall<float>&, MraPlan<float>*);
template void plan_mra<double>(const Tuning&, const InvCall<double>&, MraPlan<double>*);

// ------------------------------------------------------------------------------------------------
// Continuous wavelet transform (vw_plan.h CwtPlan)
static int cwt_lds_class(int lds) {  // 0: up to 16 KiB, 1: up to 32 KiB, ...
  int cls = 0;
  for (int cap = 16 * 1024; cap < lds; cap *= 2) ++cls;
  return cls;
}

void plan_cwt(const CwtCall& c, CwtPlan* p) {
  p->fma = (c.flags & VW_FLAG_FMA) != 0;
  p->cplx = c.cplx;
  const int nv = kCwtChunkBytes / c.elem_bytes;
  const int64_t want = ((c.N + nv - 1) / nv + 63) / 64 * 64;  // whole waves covering the row
  const int threads = (int)std::min<int64_t>(want, kCwtThreads);
  const int tile = threads * nv;
  p->threads = threads; p->nv = nv; p->tile = tile;
  p->ntiles = (int)((c.N + tile - 1) / tile);
  for (int s = 0; s < c.S; ++s) {
    const int K = c.taps[s];
    if (K > kCwtMaxTaps) {
      p->error = VW_ERR_UNSUPPORTED;
      snprintf(p->msg, sizeof(p->msg), "scale %d has %d taps: more than the %d a workgroup stages", s, K, kCwtMaxTaps);
      p->order.clear();
      return;
    }
    const int chunks = cwt_chunks(threads, K, nv);
    p->order.push_back(CwtScalePlan{s, K, tile, nv, threads, chunks, chunks * kCwtChunkBytes});
  }
  std::stable_sort(p->order.begin(), p->order.end(),
                   [](const CwtScalePlan& a, const CwtScalePlan& b) { return a.taps > b.taps; });
  for (int i = 0; i < c.S;) {
    int n = 1;
    while (i + n < c.S && cwt_lds_class(p->order[i + n].lds) == cwt_lds_class(p->order[i].lds)) ++n;
    const int64_t work = (int64_t)n * p->ntiles * c.B;
    p->launches.push_back(CwtLaunch{i, n, p->order[i].lds, (int)std::min<int64_t>(work, kCwtMaxGrid)});
    i += n;
  }
}

void plan_icwt(const IcwtCall& c, IcwtPlan* p) {
  p->fma = (c.flags & VW_FLAG_FMA) != 0;
  const int nv = kCwtChunkBytes / c.elem_bytes;
  const int64_t want = ((c.N + nv - 1) / nv + 63) / 64 * 64;  // whole waves covering the row, as plan_cwt
  const int threads = (int)std::min<int64_t>(want, kCwtThreads);
  const int tile = threads * nv;
  p->threads = threads; p->nv = nv; p->tile = tile;
  p->ntiles = (int)((c.N + tile - 1) / tile);
  for (int j = 0; j < c.nsc; ++j) {
    const int K = c.taps[j];
    if (K > kCwtMaxTaps) {
      p->error = VW_ERR_UNSUPPORTED;
      snprintf(p->msg, sizeof(p->msg), "scale %d has %d taps: more than the %d a workgroup stages", j, K, kCwtMaxTaps);
      return;
    }
    p->max_taps = std::max(p->max_taps, K);
  }
  p->chunks = cwt_chunks(threads, p->max_taps, nv);
  p->lds = p->chunks * kCwtChunkBytes;
  p->grid = (int)std::min<int64_t>((int64_t)p->ntiles * c.B, kCwtMaxGrid);
}

template <typename T>
void plan_forward(const Tuning& tu, const FwdCall<T>& c, FwdPlan<T>* p) {
  const int Lmax = std::max(c.L, hi_taps(c)), taps = listed_taps(tu, Lmax, c.L != hi_taps(c));
  if ((tu.bi & 1) && c.L != hi_taps(c) && !c.hist) {  // the two-length route where it applies (vw_plan.h)
    plan_forward_taps(tu, c, Lmax, p, true);
    if (p->error != VW_OK || p->args.taps_hi != p->args.taps) return;  // (a mixed FFT-switch level: refused on either route)
    *p = FwdPlan<T>();
  }
  plan_forward_taps(tu, c, taps, p);
  if (p->error != VW_OK && taps != Lmax) {
    *p = FwdPlan<T>();
    plan_forward_taps(tu, c, Lmax, p);
  }
}

template <typename T>
void plan_inverse(const Tuning& tu, const InvCall<T>& c, InvPlan<T>* p) {
  const int Lmax = std::max(c.L, hi_taps(c)), taps = listed_taps(tu, Lmax, c.L != hi_taps(c));
  if ((tu.bi & 2) && c.L != hi_taps(c)) {  // the two-length route where it applies (vw_plan.h), else the padded route below
    plan_inverse_taps(tu, c, Lmax, p, true);
    if (p->error == VW_OK && p->args.taps_hi != p->args.taps) return;
    *p = InvPlan<T>();
  }
  plan_inverse_taps(tu, c, taps, p);
  if (p->error != VW_OK && taps != Lmax) {
    *p = InvPlan<T>();
    plan_inverse_taps(tu, c, Lmax, p);
  }
}

// ------------------------------------------------------------------------------------------------
// Forward -> inverse pairs (vw_plan.h pair_fusable).
static bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

template <typename T>
bool pair_fusable(const FwdCall<T>& fc, const FwdPlan<T>& fp, const InvCall<T>& ic, const InvPlan<T>& ip) {
  if (sizeof(T) != 8) return false;
  if (fp.error != VW_OK || ip.error != VW_OK || !fp.fused || !ip.fused) return false;
  const int64_t B = fc.B, N = fc.N;
  const int J = fc.J, L = fc.L;
  // the two calls describe one round trip
  if (ic.B != B || ic.N != N || ic.J != J || ic.L != L || hi_taps(fc) != L || hi_taps(ic) != L) return false;
  if (fc.boundary != VW_PERIODIC || ic.boundary != VW_PERIODIC || fc.single_level || ic.single_level) return false;
  if (fp.fma != ip.fma) return false;
  if ((const T*)fc.details != ic.details || (const T*)fc.approx != ic.approx) return false;
  const unsigned all = J >= 32 ? ~0u : (1u << J) - 1u;
  if ((ic.detail_mask & all) != all || ic.approx_zero || ic.thr) return false;
  const unsigned off = VW_FLAG_VALIDATE | VW_FLAG_REF_NONFINITE | VW_FLAG_HOST_MEMORY;
  if ((fc.flags | ic.flags) & off) return false;
  if (fc.hist || fp.validate || fp.ref_nf || ip.ref_nf || fp.snapshot) return false;
  // the forward: k_forward_persist's full-slab form, a tap count k_roundtrip is instantiated for
  if (fp.kernel != kFwdPersist || !fp.args.level_ct || fp.nv != 4 || fp.args.region1 <= 0) return false;
  if (L > kPairMaxTaps || !has_unrolled_taps(L) || fp.args.taps != L || fp.args.taps_hi != L) return false;
  // the inverse: the PLAIN class, in one buffer or in the two a small batch gets
  const InvArgs<T>& ia = ip.args;
  if (ip.threads != fp.threads || ip.nv != 4 || ia.taps != L || ia.taps_hi != L) return false;
  if (!ia.plain && !(ip.kernel == kInvDb && plain_class(ic, ip, ip.nv))) return false;
  // the inverse half works in a forward level region, from the region's first element on
  for (int j = 0; j < J; ++j)
    if (ia.lv[j].s != fp.args.lv[j].s || N + ia.lv[j].hr > fp.args.region1) return false;
  if (fp.lds < 2 * fp.args.region1 * (int)sizeof(T)) return false;
  // y is written while x and the coefficient planes of later rows are still to be read
  const size_t row = (size_t)N * sizeof(T), plane = (size_t)B * row;
  const size_t x_bytes = ((size_t)(B - 1) * (size_t)fc.ldx + (size_t)N) * sizeof(T);
  if (ranges_overlap(ic.y, plane, fc.x, x_bytes) || ranges_overlap(ic.y, plane, fc.details, (size_t)J * plane) ||
      ranges_overlap(ic.y, plane, fc.approx, plane))
    return false;
  return true;
}
template bool pair_fusable<float>(const FwdCall<float>&, const FwdPlan<float>&, const InvCall<float>&,
                                  const InvPlan<float>&);
template bool pair_fusable<double>(const FwdCall<double>&, const FwdPlan<double>&, const InvCall<double>&,
                                   const InvPlan<double>&);

int pair_keep_variant(int requested, const int (&per_cu)[kPairMaxKeep + 1]) {
  if (requested >= 0) return std::min(requested, kPairMaxKeep);
  int v = kPairAutoKeep;
  while (v > 0 && per_cu[v] < per_cu[0]) --v;
  return v;
}

template void plan_forward<float>(const Tuning&, const FwdCall<float>&, FwdPlan<float>*);
template void plan_forward<double>(const Tuning&, const FwdCall<double>&, FwdPlan<double>*);
template void plan_inverse<float>(const Tuning&, const InvCall<float>&, InvPlan<float>*);
template void plan_inverse<double>(const Tuning&, const InvCall<double>&, InvPlan<double>*);

}  // namespace vw
