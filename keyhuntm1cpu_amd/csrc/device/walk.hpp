// The giant-step walks around one group's centre and what drives them, scan_batch and scan_group.
#pragma once
#include "scan_args.hpp"
#include "probe_queue.hpp"
#include "addr_point.hpp"
#include "baby_point.hpp"

namespace khbk {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// Prefix-scratch stream (written once by the forward pass, read once by the walk ~512 steps later, from
// HBM: ~35 GB per slot at 262,144 lanes).  Non-temporal loads and stores keep it from displacing the level-0 gate's L2-sized
// stage-1 fold (khb_set_gate_stage1): -1.5 % time with two launches in flight, -0.3 % as one launch
// (profiles/r04i/nt_ab.txt, r04h/ntall_ab.txt).  Without the fold (round 1, 4 waves/SIMD) they measured
// slower (profiles/r01_gate_experiments_raw.txt); tools/experiments/plainscr_patch.py builds the plain form.
__device__ __forceinline__ void scr_st(Fe* p, const Fe& v) {
  v4u* q = reinterpret_cast<v4u*>(p);
  __builtin_nontemporal_store(v4u{v.v[0], v.v[1], v.v[2], v.v[3]}, q);
  __builtin_nontemporal_store(v4u{v.v[4], v.v[5], v.v[6], v.v[7]}, q + 1);
}
__device__ __forceinline__ Fe scr_ld(const Fe* p) {
  const v4u* q = reinterpret_cast<const v4u*>(p);
  const v4u lo = __builtin_nontemporal_load(q), hi = __builtin_nontemporal_load(q + 1);
  return Fe{{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}};
}

// GSn / _2GSn rows (wave-uniform index), read through the constant address space, so rows arrive
// by scalar loads into SGPRs (lgkmcnt) instead of taking 16 VGPRs and four vector-memory slots per
// backward step.
struct GsnTable {
  const AffPt* p;
  typedef const __attribute__((address_space(4))) uint32_t* CW;
  __device__ __forceinline__ Fe ld(uint32_t word) const {
    CW w = (CW)p + word;
    Fe r;
#pragma unroll
    for (int k = 0; k < 8; ++k) r.v[k] = w[k];
    return r;
  }
  __device__ __forceinline__ Fe x(uint32_t i) const { return ld(16 * i); }
  __device__ __forceinline__ AffPt pt(uint32_t i) const { return AffPt{ld(16 * i), ld(16 * i + 8)}; }
  // p - GSn[i].x (0 for x = 0), stored after the 513 points (khb_load_giant_table)
  __device__ __forceinline__ Fe nx(uint32_t i) const { return ld(16 * KHB_GIANT_TABLE + 8 * i); }
};

// x for the probe.  With a gate only the low word of x is read before the drain, and a lazy x
// (< 2^256, congruent) differs from the canonical one only when x >= p, which needs x.v[7] ==
// 0xffffffff (p's top word): the full canonicalisation runs only then (wave-uniform skip, ~2^-26
// per wave), and the drain canonicalises its survivors before hashing.
template <int MODE>
__device__ __forceinline__ void x_out(const ScanArgs& A, Fe& x) {
  if ((MODE == kScan && A.gate) || is_gated(MODE)) {
    if (x.v[7] == 0xffffffffu) fm_canon(x, x);
  } else {
    fm_canon(x, x);
  }
}

// r = p1 + p2 given inv = 1 / (p2.x - p1.x) and, for aff_add_dy, dy = p2.y - p1.y (AddDirect, SECP256K1.cpp:242-265,
// after its inversion; inv = 0 gives the reference's result for p2.x == p1.x).  r may be p1.  Canonical in and out.
__device__ __forceinline__ void aff_add_dy(AffPt& r, const AffPt& p1, const AffPt& p2, const Fe& dy, const Fe& inv) {
  Fe s, x, y;
  fm_mul(s, dy, inv);
  fm_sqr(x, s);
  fm_sub(x, x, p1.x);
  fm_sub(x, x, p2.x);
  fm_canon(x, x);
  fm_sub(y, p2.x, x);
  fm_mul(y, y, s);
  fm_sub(y, y, p2.y);
  fm_canon(y, y);
  r.x = x;
  r.y = y;
}
__device__ __forceinline__ void aff_add(AffPt& r, const AffPt& p1, const AffPt& p2, const Fe& inv) {
  Fe dy;
  fm_sub(dy, p2.y, p1.y);
  aff_add_dy(r, p1, p2, dy, inv);
}
// AddDirect (SECP256K1.cpp:242-265) with its own inversion; used once per lane.
__device__ __forceinline__ bool add_direct(AffPt& r, const AffPt& p1, const AffPt& p2) {
  Fe dy, dx;
  fm_sub(dy, p2.y, p1.y);
  fm_sub(dx, p2.x, p1.x);
  const bool degenerate = fe_is_zero(dx);
  fm_inv(dx, dx);
  aff_add_dy(r, p1, p2, dy, dx);
  return degenerate;
}

__device__ __forceinline__ Fe fe_small(uint32_t v) {
  Fe r;
#pragma unroll
  for (int k = 0; k < 8; ++k) r.v[k] = k ? 0u : v;
  return r;
}

// The x-only step, the one copy of its arithmetic for every -m bsgs walk: x1 = x(C - GSn[i]) (pts[511 - i]) and, if
// PAIR, x2 = x(C + GSn[i]) (pts[513 + i]) from idx = 1 / (GSn[i].x - C.x), C.y, negCx = p - C.x and negCy = p - C.y, so
// every add is lazy: x = s^2 + nu, nu = nx[i] + negCx riding in the squaring's reduction (fm_sqr_add), s = (GSn.y +/-
// C.y) * idx.  Out through x_out<XMODE> to the sink with step = base + the point's index in its group: sink.first(x1) as
// soon as x1 is finished and sink.pair(x1, x2) after x2 (a sink with loads to hide issues x1's in first), or sink.one.
template <int XMODE>
__device__ __forceinline__ void x_of_slope(const ScanArgs& A, Fe& x, const Fe& gy, const Fe& cy, const Fe& idx,
                                           const Fe& nu) {
  Fe s;
  fm_add_lazy(s, gy, cy);
  fm_mul(s, s, idx);
  fm_sqr_add(x, s, nu);
  x_out<XMODE>(A, x);
}
template <int XMODE, bool PAIR, class SINK>
__device__ __forceinline__ void step_x(const ScanArgs& A, SINK& sink, const AffPt& C, const Fe& negCx,
                                       const Fe& negCy, Fe idx, int i, uint32_t base) {
  const GsnTable gsn{A.gsn};
  Fe u, x1, x2;
  const AffPt g = gsn.pt(i);
  fm_add_lazy(u, gsn.nx(i), negCx);             // nu = -(C.x + GSn.x)
  x_of_slope<XMODE>(A, x1, g.y, C.y, idx, u);
  if constexpr (PAIR) {
    sink.first(x1, base + kHalf - 1 - (uint32_t)i);
    x_of_slope<XMODE>(A, x2, g.y, negCy, idx, u);   // GSn.y - C.y
    sink.pair(x1, base + kHalf - 1 - (uint32_t)i, x2, base + kHalf + 1 + (uint32_t)i);
  } else {
    sink.one(x1, base + kHalf - 1 - (uint32_t)i);
  }
}

// The gated walks' sink: each step's two x gate-tested together (x2 absent at step 511), in the phases of
// probe_queue.hpp.  first / pair issue the step's first loads and leave it pending; the walk calls advance and finish
// behind the next step's products; one (step 511) leaves its single x pending in the same way, so every advance and
// finish of the walk has a step to work on and the loop carries no flag.  t = the point's index in its group (step_x
// is given base 0, so t stays wave-uniform; base is added when a survivor is queued).
template <int STAGES>
struct GateSink {
  const ScanArgs& A;
  ProbeQueue& Q;
  uint32_t job, base;
  GatePending G;
  __device__ __forceinline__ void first(const Fe& x1, uint32_t t1) { gate_issue_first<STAGES>(A, G, x1, t1); }
  __device__ __forceinline__ void pair(const Fe&, uint32_t, const Fe& x2, uint32_t t2) {
    gate_issue_second<STAGES>(A, G, true, x2, t2);
  }
  __device__ __forceinline__ void advance() { gate_advance<STAGES>(A, G); }
  __device__ __forceinline__ void finish() { gate_finish<STAGES>(A, Q, G, job, base); }
  __device__ __forceinline__ void one(const Fe& x1, uint32_t t1) {
    gate_issue_first<STAGES>(A, G, x1, t1);
    gate_issue_second<STAGES>(A, G, false, x1, 0);
  }
};

// The walk of kScanG* (-m bsgs with a level-0 gate), the product path: the reference's points in its backward order
// (keyhunt.cpp:3873-3943), x only, given inv = 1 / prod_{i<512} (GSn[i].x - C.x) and the forward prefix products
// P_i = prod_{k<=i} dx_k in scr (stride lanes).  For i = 511 ... 0: idx = inv * P_{i-1}, inv *= dx_i, step_x.
// The gate's two dependent round trips hide behind the next step's products: step_x leaves its step pending in the sink
// with the fold loads issued (x1's ahead of x2's arithmetic); the next step's first product (idx = inv * pre, or the
// odd step's rebuild pre * dx) runs, sink.advance tests the folds and issues the full-gate loads, the next product
// runs, and sink.finish tests the gate and queues its survivors.  Step 511 is finished by the loop's first pass, step 1
// ahead of step 0 (idx = inv: no product to hide behind) and step 0 ahead of the centre's probe: nothing is pending
// on return.
// A later step's prefix is loaded behind finish, a step (the half stream: two) ahead of its use, so its HBM latency
// hides behind a whole step and finish never has a prefetch to wait for; issued in front of the second overlapped
// product it held 8 more VGPRs through it (spills on the hot path, whose reloads waited for the gate loads at once).
// The first step is peeled and the loop's prefix load is unconditional (the half stream's last pair reloads P_1 for
// nothing), so the loop body issues the same vector-memory sequence every time and the waitcnt pass waits for exactly
// the operand it needs.
// Full stream (HALF = false): every P_i is stored; step i reads P_{i-1} and loads P_{i-2}.  Half stream
// (KHB_HALF_STREAM): only the odd P_1 ... P_509 are stored.  After the peeled step 511 the walk goes in pairs (even i,
// odd i - 1): the even step needs P_{i-1}, stored, and then loads P_{i-3}; the odd step rebuilds P_{i-2} = P_{i-3} *
// dx_{i-2} (one extra product per pair), the forward pass's own product of the same operands in the same order, so x
// is bit-identical.  Half the stream's HBM bytes (16 B per giant step instead of 32) for +4.3 % VALU.
template <int STAGES, bool HALF>
__device__ __forceinline__ void walk_gated(const ScanArgs& A, ProbeQueue& Q, const AffPt& C, Fe inv, uint32_t job,
                                           uint32_t j, const Fe* scr) {
  const size_t S = A.stride;
  const GsnTable gsn{A.gsn};
  const uint32_t base = j * KHB_GROUP;
  GateSink<STAGES> sink{A, Q, job, base};
  // the centre enters as p - C.x and p - C.y, so every per-step add/sub is a lazy add
  Fe negCx, negCy;
  fm_sub(negCx, fe_p(), C.x);
  fm_sub(negCy, fe_p(), C.y);
  Fe pre = scr_ld(scr + (size_t)(HALF ? kHalf - 3 : kHalf - 2) * S);   // P_509 / P_510
  Fe idx, dx;
  // step 511: pts[0] = C - GSn[511] only
  if constexpr (HALF) {
    fm_add_lazy(dx, gsn.x(kHalf - 2), negCx);
    fm_mul(idx, pre, dx);                                  // P_510 = P_509 * dx_510
    fm_mul(idx, inv, idx);
  } else {
    fm_mul(idx, inv, pre);
    pre = scr_ld(scr + (size_t)(kHalf - 3) * S);
  }
  fm_add_lazy(dx, gsn.x(kHalf - 1), negCx);
  fm_mul(inv, inv, dx);
  step_x<kScanG, false>(A, sink, C, negCx, negCy, idx, kHalf - 1, 0);
  if constexpr (HALF) {
    // pairs (even i, odd i - 1), i = 510 ... 2; pre = P_{i-1} on entry
    for (int i = (int)kHalf - 2; i >= 2; i -= 2) {
      fm_mul(idx, inv, pre);                                 // even step i: P_{i-1} (odd index, stored)
      sink.advance();                                        // step i + 1's folds; its gate loads
      fm_add_lazy(dx, gsn.x(i), negCx);
      fm_mul(inv, inv, dx);
      sink.finish();
      pre = scr_ld(scr + (size_t)(i > 2 ? i - 3 : 1) * S);   // P_{i-3} for step i - 1 (and i - 2); i = 2: unused
      step_x<kScanG, true>(A, sink, C, negCx, negCy, idx, i, 0);
      // odd step i - 1: P_{i-2} = P_{i-3} * dx_{i-2} (i - 1 = 1: P_0 = dx_0)
      fm_add_lazy(dx, gsn.x(i - 2), negCx);
      if (i > 2) {
        fm_mul(idx, pre, dx);
        sink.advance();                                      // step i's
        fm_mul(idx, inv, idx);
      } else {
        sink.advance();
        fm_mul(idx, inv, dx);
      }
      sink.finish();
      fm_add_lazy(dx, gsn.x(i - 1), negCx);
      fm_mul(inv, inv, dx);
      step_x<kScanG, true>(A, sink, C, negCx, negCy, idx, i - 1, 0);
    }
    sink.advance();                                                // step 1's, ahead of step 0 (idx = inv: no product)
    sink.finish();
    step_x<kScanG, true>(A, sink, C, negCx, negCy, inv, 0, 0);
  } else {
    for (int i = (int)kHalf - 2; i >= 0; --i) {
      if (i > 0) {
        fm_mul(idx, inv, pre);
        sink.advance();                                         // step i + 1's folds; its gate loads
        fm_add_lazy(dx, gsn.x(i), negCx);
        fm_mul(inv, inv, dx);
        sink.finish();
        pre = scr_ld(scr + (size_t)(i >= 2 ? i - 2 : 0) * S);   // i = 1: a harmless reload of prefix 0
      } else {
        sink.advance();
        sink.finish();
        idx = inv;
      }
      step_x<kScanG, true>(A, sink, C, negCx, negCy, idx, i, 0);
    }
  }
  sink.advance();                                // step 0's: nothing is pending past here
  sink.finish();
  probe<false>(A, Q, C.x, job, j, kHalf);        // the centre, pts[512]
}

// The names the rest of the project (bench.py's operation count) knows the two forms by.
template <int STAGES>
__device__ __forceinline__ void walk_group_g(const ScanArgs& A, ProbeQueue& Q, const AffPt& C, const Fe& inv,
                                             uint32_t job, uint32_t j, const Fe* scr) {
  walk_gated<STAGES, false>(A, Q, C, inv, job, j, scr);
}
template <int STAGES>
__device__ __forceinline__ void walk_group_g_half(const ScanArgs& A, ProbeQueue& Q, const AffPt& C, const Fe& inv,
                                                  uint32_t job, uint32_t j, const Fe* scr) {
  walk_gated<STAGES, true>(A, Q, C, inv, job, j, scr);
}

// The ungated walk's sink: level-1 probe of both x (kScan) or the x dump (kDump); t = the point's index in its group.
template <int MODE>
struct ProbeSink {
  const ScanArgs& A;
  ProbeQueue& Q;
  uint32_t job, j;
  __device__ __forceinline__ void first(const Fe&, uint32_t) const {}
  __device__ __forceinline__ void pair(const Fe& x1, uint32_t t1, const Fe& x2, uint32_t t2) const {
    if constexpr (MODE == kScan)            // both x before either probe load is issued
      asm volatile("" ::"v"(x1.v[0]), "v"(x2.v[0]), "v"(x1.v[7]), "v"(x2.v[7]) : "memory");
    probe_pair<MODE == kDump>(A, Q, x1, x2, job, j, t1, t2);
  }
  __device__ __forceinline__ void one(const Fe& x1, uint32_t t1) const { probe<MODE == kDump>(A, Q, x1, job, j, t1); }
};
// The ungated x-only walk (kScan, kDump): walk_gated's points and order over the full stream, every x probed or dumped;
// C is canonical, products are lazy and every x is canonicalised before it is hashed or dumped (x_out<MODE>).
template <int MODE>
__device__ __forceinline__ void walk_group_x(const ScanArgs& A, ProbeQueue& Q, const AffPt& C, Fe inv, uint32_t job,
                                             uint32_t j, const Fe* scr) {
  static_assert(is_batched(MODE) && !is_gated(MODE), "walk_group_x: kScan or kDump (called from scan_batch)");
  const size_t S = A.stride;
  const GsnTable gsn{A.gsn};
  const ProbeSink<MODE> sink{A, Q, job, j};
  Fe negCx, negCy;
  fm_sub(negCx, fe_p(), C.x);
  fm_sub(negCy, fe_p(), C.y);
  Fe pre = scr_ld(scr + (size_t)(kHalf - 2) * S), idx, dx;
  fm_mul(idx, inv, pre);
  pre = scr_ld(scr + (size_t)(kHalf - 3) * S);
  fm_add_lazy(dx, gsn.x(kHalf - 1), negCx);
  fm_mul(inv, inv, dx);
  step_x<MODE, false>(A, sink, C, negCx, negCy, idx, kHalf - 1, 0);
  for (int i = (int)kHalf - 2; i >= 0; --i) {
    if (i > 0) {
      fm_mul(idx, inv, pre);
      pre = scr_ld(scr + (size_t)(i >= 2 ? i - 2 : 0) * S);
      fm_add_lazy(dx, gsn.x(i), negCx);
      fm_mul(inv, inv, dx);
    } else {
      idx = inv;
    }
    step_x<MODE, true>(A, sink, C, negCx, negCy, idx, i, 0);
  }
  probe<MODE == kDump>(A, Q, C.x, job, j, kHalf);
}

// The x,y walk's sink (-m address, kBaby).
template <int MODE>
__device__ __forceinline__ void point_xy(const ScanArgs& A, const Fe& x, const Fe& y, uint32_t job, uint32_t j,
                                         uint32_t t) {
  if constexpr (MODE == kBaby)
    baby_point(A, x, job, j, t);
  else
    addr_point<MODE>(A, x, y, job, j, t);
}
// walk_group_x's points and order with y where the mode hashes it (needs_y), canonical, to point_xy; plain loads.
// (-m xpoint without -e walks x only, walk_group_ax below.)
template <int MODE>
__device__ __forceinline__ void walk_group_xy(const ScanArgs& A, const AffPt& C, Fe inv, uint32_t job, uint32_t j,
                                              const Fe* scr) {
  static_assert(is_xy(MODE), "walk_group_xy: an -m address mode or kBaby (called from scan_group)");
  const uint32_t S = A.stride;
  const GsnTable gsn{A.gsn};
  Fe pre, dx;
  for (int i = (int)kHalf - 1; i >= 0; --i) {
    Fe idx;
    if (i > 0) {
      pre = scr[(size_t)(i - 1) * S];
      fm_mul(idx, inv, pre);
      const Fe gx = gsn.x(i);
      fm_sub(dx, gx, C.x);
      fm_mul(inv, inv, dx);
    } else {
      idx = inv;
    }
    Fe u, s, x1, y1;
    const AffPt g = gsn.pt(i);
    fm_add(u, C.x, g.x);                  // x = s^2 - (C.x + GSn.x)
    // C - GSn[i]: s = (-GSn.y - C.y)/dx; x needs only s^2, and with s' = -s = (GSn.y + C.y)/dx
    // y = (GSn.x - x)*s + GSn.y = (x - GSn.x)*s' + GSn.y   (keyhunt.cpp:2628-2641)
    fm_add(s, g.y, C.y);
    fm_mul(s, s, idx);
    fm_sqr(x1, s);
    fm_sub(x1, x1, u);
    x_out<MODE>(A, x1);
    if constexpr (needs_y(MODE)) {
      Fe t;
      fm_sub(t, x1, g.x);
      fm_mul(t, t, s);
      fm_canon(t, t);
      fm_add(y1, t, g.y);
    }
    if (i < (int)kHalf - 1) {
      // C + GSn[i]: s = (GSn.y - C.y)/dx; y = (GSn.x - x)*s - GSn.y   (keyhunt.cpp:2611-2624)
      Fe x2, y2;
      fm_sub(s, g.y, C.y);
      fm_mul(s, s, idx);
      fm_sqr(x2, s);
      fm_sub(x2, x2, u);
      x_out<MODE>(A, x2);
      if constexpr (needs_y(MODE)) {
        fm_sub(y2, g.x, x2);
        fm_mul(y2, y2, s);
        fm_sub(y2, y2, g.y);
        fm_canon(y2, y2);
      }
      point_xy<MODE>(A, x1, y1, job, j, kHalf - 1 - (uint32_t)i);
      point_xy<MODE>(A, x2, y2, job, j, kHalf + 1 + (uint32_t)i);
    } else {
      point_xy<MODE>(A, x1, y1, job, j, kHalf - 1 - (uint32_t)i);
    }
  }
  point_xy<MODE>(A, C.x, C.y, job, j, kHalf);
}

// The x-only walk's sink for -m xpoint: each step's two x serialised and probed together (addr_point.hpp).
template <int MODE>
struct XPointSink {
  const ScanArgs& A;
  uint32_t job, j;
  __device__ __forceinline__ void first(const Fe&, uint32_t) const {}
  __device__ __forceinline__ void pair(const Fe& x1, uint32_t t1, const Fe& x2, uint32_t t2) const {
    // both x before either bloom load is issued
    asm volatile("" ::"v"(x1.v[3]), "v"(x2.v[3]), "v"(x1.v[7]), "v"(x2.v[7]) : "memory");
    xpoint_probe<MODE, true>(A, x1, t1, x2, t2, job, j);
  }
  __device__ __forceinline__ void one(const Fe& x1, uint32_t t1) const {
    xpoint_probe<MODE, false>(A, x1, t1, x1, t1, job, j);
  }
};
// The x-only walk of -m xpoint inside scan_group's scheme: walk_group_x's points, order and step (step_x: lazy adds,
// fm_sqr_add, the nx rows by scalar loads) over scan_group's prefixes P_0 ... P_510 (plain loads, one step ahead), y
// never computed; every x canonical before it is serialised (x_out<MODE>), so bit-identical to walk_group_xy's.
// The steps read C.x only as p - C.x, so C.x gives up its 8 VGPRs for the walk and is rebuilt after it: C.x is
// canonical and not 0 (no point of the curve has x = 0), so both subtractions are exact, without a borrow.
template <int MODE>
__device__ __forceinline__ void walk_group_ax(const ScanArgs& A, AffPt& C, Fe inv, uint32_t job, uint32_t j,
                                              const Fe* scr) {
  static_assert(MODE == kAddrX, "walk_group_ax: kAddrX (called from scan_group)");
  const size_t S = A.stride;
  const GsnTable gsn{A.gsn};
  const XPointSink<MODE> sink{A, job, j};
  Fe negCx, negCy;
  fm_sub(negCx, fe_p(), C.x);
  fm_sub(negCy, fe_p(), C.y);
  Fe pre = scr[(size_t)(kHalf - 2) * S], idx, dx;
  fm_mul(idx, inv, pre);
  pre = scr[(size_t)(kHalf - 3) * S];
  fm_add_lazy(dx, gsn.x(kHalf - 1), negCx);
  fm_mul(inv, inv, dx);
  step_x<MODE, false>(A, sink, C, negCx, negCy, idx, kHalf - 1, 0);
  for (int i = (int)kHalf - 2; i >= 0; --i) {
    if (i > 0) {
      fm_mul(idx, inv, pre);
      pre = scr[(size_t)(i >= 2 ? i - 2 : 0) * S];
      fm_add_lazy(dx, gsn.x(i), negCx);
      fm_mul(inv, inv, dx);
    } else {
      idx = inv;
    }
    step_x<MODE, true>(A, sink, C, negCx, negCy, idx, i, 0);
  }
  fm_sub(C.x, fe_p(), negCx);
  sink.one(C.x, kHalf);
}

// One reference group centred on C, walked on its own (-m address, baby steps): the 513-element
// batch of IntGroup.cpp:36-58 including dx[512] = _2GSn.x - C.x, whose inverse advances C to the
// next centre (keyhunt.cpp:3986-3999).  For -m address this is keyhunt.cpp:2586-2711 with the
// table Gn (same point order t = 0..1023, pts[t] = key + t), plus y where the search needs it.
template <int MODE>
__device__ __forceinline__ void scan_group(const ScanArgs& A, AffPt& C, uint32_t job, uint32_t j, Fe* scr) {
  const uint32_t S = A.stride;
  // GSn rows are wave-uniform: read them through the constant address space so they arrive by
  // scalar loads (SGPRs, lgkmcnt) instead of occupying 16 VGPRs and the vector-memory queue.
  const GsnTable gsn{A.gsn};
  Fe acc, dx;
  // forward pass: prefix products of dx[i] = GSn[i].x - C.x (i < 512) and _2GSn.x - C.x
  {
    const Fe gx = gsn.x(0);
    fm_sub(acc, gx, C.x);
  }
  scr[0] = acc;
  for (uint32_t i = 1; i < kHalf; ++i) {
    const Fe gx = gsn.x(i);
    fm_sub(dx, gx, C.x);
    fm_mul(acc, acc, dx);
    scr[(size_t)i * S] = acc;
  }
  {
    const Fe gx = gsn.x(kHalf);
    fm_sub(dx, gx, C.x);
  }
  fm_mul(acc, acc, dx);
  Fe accc;
  fm_canon(accc, acc);
  const bool degenerate = fe_is_zero(accc);
  Fe inv;
  fm_inv(inv, acc);                       // == 0 (mod p) when degenerate -> every inverse 0, as the reference
  {
    // i = 512's inverse is only needed for the next centre: park it in prefix slot 511, which
    // is read exactly once (here), instead of holding 8 VGPRs through the backward loop.
    Fe inv2;
    const Fe pre = scr[(size_t)(kHalf - 1) * S];
    fm_mul(inv2, inv, pre);
    scr[(size_t)(kHalf - 1) * S] = inv2;
    asm volatile("" ::: "memory");
  }
  fm_mul(inv, inv, dx);
  // -m xpoint walks x only (4.8 % less kernel time than walk_group_xy<kAddrX>, profiles/xpoint).  With -e the point
  // handler holds two more field elements and the x-only walk spilled at 3 waves per SIMD (16 B of scratch; none
  // with walk_group_xy, whose y is not computed either: needs_y), so kAddrXE keeps the x,y walk's form.
  if constexpr (MODE == kAddrX)
    walk_group_ax<MODE>(A, C, inv, job, j, scr);
  else
    walk_group_xy<MODE>(A, C, inv, job, j, scr);
  // next centre: C + _2GSn with y (keyhunt.cpp:3986-3999)
  {
    asm volatile("" ::: "memory");
    const Fe inv2 = scr[(size_t)(kHalf - 1) * S];
    aff_add(C, C, gsn.pt(kHalf), inv2);
  }
  if (!is_dump(MODE) && degenerate) emit_degen(A, job, j);
}

// -m bsgs work item: groups [g0, g1) (at most kBatch) of one job with TWO field inversions in
// total instead of one per group plus one per lane start:
//  0. centres C_g = startP + gofs[g0+g] (gofs[j] = j*_2GSn), all from startP, batch-inverted
//     together (Montgomery over the <= kBatch x-differences; AddDirect, SECP256K1.cpp:242-265);
//  1. per group the forward prefix products of dx_i = GSn[i].x - C.x, i < 512, into scratch;
//     the group totals T_g are chained into one product;
//  2. one inversion of that product, split back into inv(T_g) (Montgomery again);
//  3. per group the reference's backward walk (walk_group_g_half / walk_group_g / walk_group_x).
// The reference's batch per group also holds dx[512] = _2GSn.x - C.x (the next-centre add); its
// inverse is not needed here (centres come from step 0), but a group whose 513-element product is
// zero gets all-zero inverses in the reference (IntGroup.cpp:36-58 + IntMod.cpp:497-500): such a
// group is kept out of the chained product and walked with inv = 0, which reproduces its x values
// bit for bit (and is reported, as scan_group does).
// Scratch (lane-private, stride = lanes, 32 B entries): g*512 + i (i < 511) prefixes of group g,
// g*512 + 511 = T_g then inv(T_g); kBatch*512 + 2g (+1) = C_g.x (.y); kBatch*514 + g = chained
// products.
template <int MODE>
__device__ __forceinline__ uint32_t scan_batch(const ScanArgs& A, ProbeQueue& Q, uint32_t job, uint32_t g0,
                                               uint32_t g1, Fe* scr) {
  static_assert(is_batched(MODE), "scan_batch: a -m bsgs mode (kScan, kScanG*, kDump)");
  const size_t S = A.stride;
  const GsnTable gsn{A.gsn};
  const uint32_t nb = g1 - g0;
  Fe* const sc = scr + (size_t)kBatch * kHalf * S;          // centres
  Fe* const sq = scr + (size_t)kBatch * (kHalf + 2) * S;    // chained products
  const AffPt P = A.centres[job];
  // 0. centres
  uint32_t skip = 0;      // bit g: no add (group 0 is startP) or a degenerate add (gofs.x == P.x)
  Fe acc;
  for (uint32_t g = 0; g < nb; ++g) {
    const uint32_t jg = g0 + g;
    Fe d = fe_small(1);
    if (jg != 0) {
      fm_sub(d, A.gofs[jg].x, P.x);
      Fe dc;
      fm_canon(dc, d);
      if (fe_is_zero(dc)) {
        d = fe_small(1);
        skip |= 1u << g;
        if (MODE != kDump) emit_degen(A, job, jg | 0x80000000u);
      }
    } else {
      skip |= 1u << g;
    }
    if (g == 0) acc = d; else fm_mul(acc, acc, d);
    sq[g * S] = acc;
  }
  Fe inv;
  fm_inv(inv, acc);
  for (int g = (int)nb - 1; g >= 0; --g) {
    const uint32_t jg = g0 + (uint32_t)g;
    const AffPt O = A.gofs[jg];
    Fe ig;
    if (g > 0) {
      fm_mul(ig, inv, sq[(g - 1) * S]);
      Fe d = fe_small(1);
      if (!((skip >> g) & 1u)) fm_sub(d, O.x, P.x);
      fm_mul(inv, inv, d);
    } else {
      ig = inv;
    }
    AffPt C = P;
    if (jg != 0) {
      if ((skip >> g) & 1u) ig = fe_small(0);      // as add_direct: inverse of 0 is 0
      Fe s, x, y;                                  // C = P + O: aff_add(C, P, O, ig) written out
      fm_sub(s, O.y, P.y);
      fm_mul(s, s, ig);
      fm_sqr(x, s);
      fm_sub(x, x, P.x);
      fm_sub(x, x, O.x);
      fm_canon(x, x);
      fm_sub(y, O.x, x);
      fm_mul(y, y, s);
      fm_sub(y, y, O.y);
      fm_canon(y, y);
      C.x = x;
      C.y = y;
    }
    sc[2 * g * S] = C.x;
    sc[(2 * g + 1) * S] = C.y;
  }
  // 1. forward passes
  const Fe g2x = gsn.x(kHalf);
  uint32_t degen = 0;
  for (uint32_t g = 0; g < nb; ++g) {
    Fe* const sg = scr + (size_t)g * kHalf * S;
    const Fe cx = sc[2 * g * S];
    Fe a, dx, negCx;
    fm_sub(negCx, fe_p(), cx);
    // dx_i = GSn[i].x - C.x as the lazy sum GSn[i].x + (p - C.x) (congruent; feeds products only)
    fm_add_lazy(a, gsn.x(0), negCx);
    if (!(kHalfStream && is_gated(MODE))) scr_st(sg, a);       // P_0 is not stored by the half stream
    for (uint32_t i = 1; i < kHalf - 1; ++i) {
      fm_add_lazy(dx, gsn.x(i), negCx);
      fm_mul(a, a, dx);
      if (!(kHalfStream && is_gated(MODE)) || (i & 1u)) scr_st(sg + i * S, a);
    }
    fm_add_lazy(dx, gsn.x(kHalf - 1), negCx);
    fm_mul(a, a, dx);
    Fe ac;
    fm_canon(ac, a);
    if (fe_is_zero(ac) || fe_eq(g2x, cx)) {
      degen |= 1u << g;
      a = fe_small(1);
    }
    sg[(kHalf - 1) * S] = a;
    if (g == 0) acc = a; else fm_mul(acc, acc, a);
    sq[g * S] = acc;
  }
  // 2. one inversion for the batch
  fm_inv(inv, acc);
  for (int g = (int)nb - 1; g >= 0; --g) {
    Fe* const sg = scr + (size_t)g * kHalf * S;
    Fe ig;
    if (g > 0) {
      fm_mul(ig, inv, sq[(g - 1) * S]);
      fm_mul(inv, inv, sg[(kHalf - 1) * S]);
    } else {
      ig = inv;
    }
    if ((degen >> g) & 1u) ig = fe_small(0);
    sg[(kHalf - 1) * S] = ig;
  }
  // 3. backward walks
  uint32_t walked = 0;
  for (uint32_t g = 0; g < nb; ++g, ++walked) {
    Fe* const sg = scr + (size_t)g * kHalf * S;
    asm volatile("" ::: "memory");
    const AffPt C{sc[2 * g * S], sc[(2 * g + 1) * S]};
    if constexpr (is_gated(MODE) && kHalfStream)
      walk_group_g_half<gate_stages(MODE)>(A, Q, C, sg[(kHalf - 1) * S], job, g0 + g, sg);
    else if constexpr (is_gated(MODE))
      walk_group_g<gate_stages(MODE)>(A, Q, C, sg[(kHalf - 1) * S], job, g0 + g, sg);
    else
      walk_group_x<MODE>(A, Q, C, sg[(kHalf - 1) * S], job, g0 + g, sg);
    if (MODE != kDump && ((degen >> g) & 1u)) emit_degen(A, job, g0 + g);
  }
  return walked;
}

}  // namespace khbk
