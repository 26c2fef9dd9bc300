// gtop_interval_tree.h — the refinement tree of the continuous-time certificates, device-only, stated
// once for gtop_certify.hip (clearance: the static field, and the field with the moving boxes) and gtop_kinematics.hip
// (velocity and acceleration).  tests/interval_tree_twin.py is its numpy restatement.
//
// One WAVEFRONT per trajectory, no workgroup barrier, nothing per interval to HBM.  A segment is cut into 64 intervals,
// one per lane; an interval that is neither certified nor in violation is OPEN and is replaced by its 64 children,
// depth-first in ascending time, while the depth and the trajectory's refinement budget allow.  A certificate says what
// it adds as a NODE:
//   typename NODE::Bound                  what an interval's evaluation leaves for its leaf
//   int  eval(a, w, lane, Bound &)        the interval [a, a + w] of the lane: its status; the midpoint's figures go
//                                         into the node's running results at every level
//   void leaf(const Bound &)              the interval stays in the tree: commit its bound
#pragma once

#include <hip/hip_runtime.h>

#include "gtop_kernels.h"   // GTOP_CERT_MAX_DEPTH

// The interval's ends are unfused, as the certificates' own arithmetic is: a numpy restatement reproduces the bits.  The
// pragma holds to the end of the translation unit: a certificate's file includes this header last, after its own
// `#pragma clang fp contract(off)`, so that the headers whose expressions fuse (poly_vel, the lookup) stay as they are.
#pragma clang fp contract(off)

enum { kCertified = 0, kOpen = 1, kViolation = 2 };

// Level L of the refinement: the 64 intervals [base + j w, base + (j + 1) w], lane j's its own; then the OPEN ones in
// ascending time, each replaced by its children while the depth and the budget allow.  nref and nund are wave-uniform.
// max_depth and max_refine are read where the caller keeps them (by value, the moving kernels' copies, which live in LDS
// because the scalar file is full, would each take a scalar register for the whole walk: 6 more SGPRs in those kernels).
template <int L, class NODE>
__device__ __forceinline__ void gtop_tree_level(NODE &N, const int &max_depth, const int &max_refine, double base,
                                                double w, int lane, int &nref, int &nund) {
  const double a = base + (double)lane * w;
  typename NODE::Bound bound;
  const int st = N.eval(a, w, lane, bound);
  unsigned long long open = __ballot(st == kOpen);
  bool leaf = st != kOpen;
  if constexpr (L < GTOP_CERT_MAX_DEPTH) {
    const double wc = 0.015625 * w;                     // w / 64
    while (open) {                                      // wave-uniform
      const int j = __ffsll((long long)open) - 1;
      open &= open - 1;
      if (L < max_depth && nref < max_refine) {
        ++nref;
        const double aj = __shfl(a, j);                 // the interval being refined, from its lane
        gtop_tree_level<L + 1>(N, max_depth, max_refine, aj, wc, lane, nref, nund);
      } else {
        ++nund;
        leaf |= lane == j;
      }
    }
  } else {
    nund += __popcll(open);
    leaf = true;
  }
  if (leaf) N.leaf(bound);
}

// Row s of a trajectory's coefficients `cf` (18 per segment: [cx0..5 | cy0..5 | cz0..5], ascending powers) into seg_c,
// 18 doubles of LDS.  The coefficients are wave-uniform, and as scalar loads they, a kernel's other uniform values and
// the masks of four levels overflow the scalar register file (17 SGPRs spilled in the clearance kernel).  Read back
// from LDS they are vector registers.
__device__ __forceinline__ void gtop_tree_stage_segment(double *seg_c, const double *cf, int s, int lane) {
  __builtin_amdgcn_wave_barrier();                      // (LDS operations of one wavefront complete in order)
  if (lane < 18) seg_c[lane] = cf[s * 18 + lane];
  __builtin_amdgcn_wave_barrier();
}

// A row's verdict and the time of its first violation, from the earliest violating midpoint (INFINITY: none) and the
// OPEN intervals left in the tree.
__device__ __forceinline__ double gtop_tree_verdict(double viol_t, int nund) {
  return viol_t != INFINITY ? -1.0 : (nund == 0 ? 1.0 : 0.0);
}
__device__ __forceinline__ double gtop_tree_first_violation(double viol_t) { return viol_t != INFINITY ? viol_t : -1.0; }
