// gtop_launch_rule.h — the launch rule of gtop_eval_wave_kernel and the ONE statement of its LDS layout: the kernel
// (gtop_wave_kernel.h) takes its offsets from the functions below, the launcher (gtop_kernels.hip) its LDS size from
// their sum.  No HIP header: gtop_launch_rule.cpp builds with a host compiler alone (tests/test_launch_rule.py).
#ifndef GTOP_LAUNCH_RULE_H_
#define GTOP_LAUNCH_RULE_H_

#include <stddef.h>

#ifdef __HIPCC__
#define GTOP_HD __host__ __device__
#else
#define GTOP_HD
#endif

// How one launch is laid out on the wavefronts: spl = samples per lane (3: ten lanes per segment, one trajectory of up
// to 6 segments per wavefront; 6: five lanes per segment, up to 12 segments), nt = trajectories per wavefront (2 only
// at spl 6 with up to 6 segments), is_long = more than 12 segments (the wavefront walks them 12 at a time).
struct GtopEvalPlan {
  int spl, nt;
  bool is_long;
  int nw;   // wavefronts per trajectory: 2 for 7 .. 12 segments at ten lanes per segment (small batches), else 1
  // which gradient the bodies compute (gtop_set_gradient_mode): 0 the reference's callback, 1 the consistent one.  The
  // launch rule leaves it 0 and does not look at it — both modes have a body for every geometry; the caller sets it.
  int consistent;
};
// The launch rule.  pinned_spl: 0 = auto, 3 or 6; for_optimizer: the optimizer loop and the evaluations of its
// multi-launch forms (the same rule with the loop's own switch point to two trajectories per wavefront).  false: the request cannot be served (m < 2, spl 3 with more than 6
// segments, more segments than one wavefront's LDS holds — past 227, in the optimizer loop past 118).
bool gtop_eval_plan(int B, int m, size_t elem, int pinned_spl, bool for_optimizer, GtopEvalPlan *plan);
// the launch rule restricted to the geometries that have a moving-term body; false: none serves the request
bool gtop_eval_plan_moving(int B, int m, int pinned_spl, bool for_optimizer, GtopEvalPlan *plan);

// ---- the LDS of one workgroup, in elements of the launch's arithmetic type (the optimizer loop: doubles):  tile [tile
// rows][stride] | gradient rows | per trajectory: x, xcur, xprev, xprevprev, dfdx, sigma, lb, ub [rows] each, Df [18], T [m]
constexpr int kSamples = 30;     // src/grad_traj_optimizer.cpp:351
constexpr int kRedVals = 19;     // 18 gradient entries + 1 cost per sample
// row stride of the LDS tile: the busy lanes (LPS*SPW of 64) of the trajectory's nw wavefronts, made odd (two wavefronts
// at ten lanes per segment: 120 busy lanes)
GTOP_HD constexpr int gtop_tile_stride(int spl, int nw) { return (nw * (kSamples / spl) * (64 / (kSamples / spl))) | 1; }
// ... of the chunked body (more than 12 segments): five lanes per segment, 5 m columns, made odd
GTOP_HD constexpr int gtop_tile_stride_long(int m) { return ((kSamples / 6) * m) | 1; }
// rows of the tile (the chunked body sums the cost in registers)
GTOP_HD constexpr int gtop_tile_rows(bool is_long) { return is_long ? 18 : kRedVals; }
// rows of the optimizer loop's LDS vectors: n <= 45 resp. 99 variables; the chunked body: n made a multiple of 32 (every
// access is bounded by n: the padding only keeps the rows whole 256-byte lines apart.  A multiple of 64 put 118 segments — the
// limit include/gtop.h states — 752 bytes past 160 KiB: refused; with 32 they fit, and 119 and more still do not)
GTOP_HD constexpr int gtop_mma_rows(int spl, int nt) { return (spl == 6 && nt == 1) ? 128 : 64; }
GTOP_HD constexpr int gtop_mma_rows_long(int n) { return (n + 31) & ~31; }   // n = 9 (m - 1) free variables
// the gradient rows between the tile and the state: [rounds * 64] <= 128 (the chunked body: one vector)
GTOP_HD constexpr int gtop_grad_rows(bool is_long, int rows) { return is_long ? rows : 128; }
// a trajectory's state: Df at kStateVecs * rows, T at kStateVecs * rows + kDfVals; its doubles (up to 12 segments: 18 + m <= 32)
constexpr int kStateVecs = 8;
constexpr int kDfVals = 18;       // Df: (p, v, a) at the start and at the end, three axes
GTOP_HD constexpr int gtop_state_doubles(bool is_long, int rows, int m) { return kStateVecs * rows + kDfVals + (is_long ? m + 8 : 14); }
// LDS bytes of one workgroup: the tile, the gradient rows (a plain evaluation of the chunked body has none), the loop's state
inline size_t gtop_wave_lds_bytes(const GtopEvalPlan &p, int m, size_t elem, bool mma) {
  const int stride = p.is_long ? gtop_tile_stride_long(m) : gtop_tile_stride(p.spl, p.nw);
  const int rows = p.is_long ? gtop_mma_rows_long(9 * (m - 1)) : gtop_mma_rows(p.spl, p.nt);
  const size_t tile = (size_t)gtop_tile_rows(p.is_long) * stride + ((mma || !p.is_long) ? gtop_grad_rows(p.is_long, rows) : 0);
  return (tile + (mma ? (size_t)p.nt * gtop_state_doubles(p.is_long, rows, m) : 0)) * elem;
}

// WIDE = false needs 24-bit (signed) multiplicands and corner records below 4 GiB (record_loads)
inline bool gtop_field_is_narrow(int nx, int ny, int nz, size_t elem) {
  const unsigned long long nrec = (unsigned long long)(nx + 1) * (ny + 1) * (nz + 2);
  return (unsigned long long)(nx + 1) * (ny + 1) < (1ull << 23) && nz + 2 < (1 << 23) && nrec * 4 * elem < (1ull << 32);
}

#endif  // GTOP_LAUNCH_RULE_H_
