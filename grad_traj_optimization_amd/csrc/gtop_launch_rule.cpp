// gtop_launch_rule.cpp — the launch rule of the evaluation kernels (gtop_launch_rule.h): which geometry serves a batch
// of B trajectories of m segments.  Host only, no HIP; every switch point below is a measurement.
#include "gtop_launch_rule.h"

constexpr int kTwoPerWaveF64From = 4096;
constexpr int kTwoPerWaveF32From = 2048;
// The optimizer loop with two trajectories per wavefront (both states in LDS, the update once per trajectory) needs the
// two-wavefront register budget, where the plain two-per-wavefront body runs three wavefronts per SIMD.  Measured per
// pass of the loop (one box, us, one | two per wavefront): fp32 evaluations B = 2 048 5.0 | 5.2, 3 072 9.0 | 7.5,
// 4 096 11.2 | 7.6, 8 192 19.2 | 14.5, 16 384 35.8 | 28.0 — from 3 072; fp64 4 096 9.6 | 9.8, 8 192 18.4 | 18.5,
// 16 384 36.2 | 35.3: no gain, the fp64 loop stays at one per wavefront unless six samples per lane are pinned.
constexpr int kOptTwoPerWaveF32From = 3072;
constexpr int kOptTwoPerWaveF64From = 1 << 30;
// One lane per segment (SPL = 30, as many trajectories per wavefront as fit) has a quarter fewer instructions per
// trajectory than five lanes per segment — and four times the distinct 128-byte lines per load instruction (the lanes
// of an instruction are 64 different segments; five lanes of a segment share a line or two), which is what the vector
// L1 counts.  Measured (one box, us, launch rule | one lane per segment): fp64 B = 16 384 29.6 | 34.1, 65 536 113.9 |
// 130.2, 131 072 240 | 259 — never; fp32 (half the loads per sample) 16 384 23.4 | 26.1, 32 768 47.2 | 51.0, 65 536
// 85.8 | 80.1, 131 072 166 | 135 (-19 %); 12 segments fp32 32 768 82.5 | 79.2.  So: fp32 only, from B x m = 393 216.
constexpr int kThreeLanesShortFrom = 8192;   // three lanes per segment: 2 .. 5 segments from this batch, 7 .. 10 from that
constexpr int kThreeLanesMidFrom = 4096;
constexpr long long kOneLaneF32FromSegments = 65536LL * 6;
constexpr int kTwoWavesUpTo = 1024;   // trajectories of 7 .. 12 segments: two wavefronts each up to this batch (2 048 wavefronts)

// The launch rule (measured).  Up to 6 segments: ten lanes per segment, one wavefront per
// trajectory, up to 12 288 trajectories in fp64 and 8 192 in fp32, where two trajectories per wavefront at five lanes
// per segment take over (fp32: packed sample pairs).  7 .. 12 segments: five lanes per segment, one
// trajectory per wavefront.  Past 12: the same wavefront walks the segments 12 at a time (LONG).  The optimizer loop
// follows the same rule with its own switch points (elem: the precision of its evaluations).  pinned_spl = 3 or 6 overrides the lanes-per-segment choice where it can
// be honoured (3: up to 6 segments; 30 = one lane per segment: up to 12 segments, plain evaluations; by itself the rule
// takes it for fp32 batches of 65 536 six-segment trajectories and more).
bool gtop_eval_plan(int B, int m, size_t elem, int pinned_spl, bool for_optimizer, GtopEvalPlan *plan) {
  if (m < 2 || (pinned_spl != 0 && pinned_spl != 3 && pinned_spl != 6 && pinned_spl != 10 && pinned_spl != 30)) return false;
  GtopEvalPlan p{};
  p.nw = 1;
  // one lane per segment (SPL = 30; the kernel's MANY): trajectories of up to 12 segments, 64 / m of them per wavefront,
  // plain evaluation only — for batches that put several such wavefronts on every SIMD
  const bool many_ok = m <= 64 && !for_optimizer;   // (a wavefront has 64 segment slots)
  if (pinned_spl == 30 && !many_ok) return false;
  // three lanes per segment (SPL = 10): 21 segment slots per wavefront, 21 / m whole trajectories of up to 10 segments.
  // Five lanes per segment hold 12 slots — two trajectories of up to 6 segments or one of up to 12 — and leave most of a
  // wavefront idle for every length but 6, 11 and 12 (busy lanes, five | three per segment: m = 2: 20 | 60, 3: 30 | 63,
  // 4: 40 | 60, 5: 50 | 60, 6: 60 | 54, 7: 35 | 63, 8: 40 | 48, 9: 45 | 54, 10: 50 | 60, 11: 55 | 33, 12: 60 | 36).
  // Measured (one box, us, launch rule of before | three lanes per segment), B = 16 384 fp64: m = 2 27.1 | 13.3, 3 27.5 |
  // 18.5, 4 28.1 | 24.2, 5 29.1 | 25.5; fp32: 3 22.6 | 14.9, 4 22.8 | 18.4, 5 23.1 | 19.2; B = 8 192 fp64: 7 26.7 | 18.6,
  // 8 27.0 | 23.4, 9 27.2 | 23.7, 10 27.7 | 24.2; fp32: 7 21.7 | 14.7, 8 21.9 | 17.9, 10 22.1 | 18.3; B = 4 096: m = 4
  // 9.1 | 9.5, 7 14.6 | 12.9, 10 15.1 | 13.8 (fp32 7: 11.2 | 9.6); B = 3 072, m = 8: 11.5 | 12.4; 2 048: alike.
  const bool three_ok = m <= 10 && !for_optimizer;
  if (pinned_spl == 10 && !three_ok) return false;
  const bool three_auto = pinned_spl == 0 && three_ok && m != 6 &&
                          B >= (m <= 5 ? kThreeLanesShortFrom : kThreeLanesMidFrom);
  if (three_ok && (pinned_spl == 10 || three_auto) && !(pinned_spl == 0 && many_ok && elem == 4 &&
                                                        (long long)B * m >= kOneLaneF32FromSegments)) {
    p.spl = 10;
    p.nt = 21 / m;
    p.is_long = false;
    *plan = p;
    return true;
  }
  // ... and past 12 segments (up to 64: a wavefront's segment slots) where the chunked body — 12 segments at a time at
  // five lanes per segment — ends on a mostly idle chunk: 64 / m trajectories per wavefront against ceil(m / 12) chunks
  // per trajectory.  Measured (one box, us, chunked | one lane per segment, fp64): B = 8 192 m = 13 56.0 | 34.7, 17 58.4 |
  // 47.7, 22 58.8 | 61.8, 24 60.3 | 64.2, 25 83.4 | 70.5, 32 110 | 87.7, 33 110 | 109, 36 111 | 112; B = 4 096 m = 13
  // 29.8 | 24.0, 17 31.5 | 32.4, 32 60.8 | 38.9, 40 90.3 | 61.1, 48 107 | 68.5, 64 192 | 87.6; B = 2 048 m = 13 15.5 | 19.6,
  // 17 16.6 | 21.2, 32 39.4 | 25.5; fp32 B = 8 192 m = 13 43.9 | 23.6, 17 45.2 | 33.9, 24 46.1 | 43.0, 32 65.6 | 48.4, 36 66.1
  // | 78.1.  So: when (trajectories per wavefront) x (chunks) >= 5, or from four chunks, and the batch gives every SIMD
  // a wavefront.
  bool many_long = false;
  if (pinned_spl == 0 && many_ok && m > 12) {
    const int nt30 = 64 / m, chunks = (m + 11) / 12;
    many_long = (nt30 * chunks >= 5 || chunks >= 4) && B >= 1024 * nt30;
  }
  if (many_ok && (pinned_spl == 30 || many_long ||
                  (pinned_spl == 0 && m <= 12 && elem == 4 && (long long)B * m >= kOneLaneF32FromSegments))) {
    p.spl = 30;
    p.nt = 64 / m;
    p.is_long = false;
    if (gtop_wave_lds_bytes(p, m, elem, false) > 160u * 1024u) return false;
    *plan = p;
    return true;
  }
  // (two trajectories per wavefront at five lanes per segment amortise the per-lane set-up — coefficients, jerk term,
  // A^-T — over six samples instead of three: fewer instructions per trajectory, longer chains per wavefront; it wins
  // once the batch puts several wavefronts on every SIMD.  Round 4, corner records and the sample's loads issued
  // together (one box, us, ten lanes | five lanes per segment): fp64 B = 3 072 8.0 | 9.1, 4 096 10.4 | 9.7, 8 192 18.6 |
  // 16.9, 16 384 36.9 | 30.7 — from 4 096 (round 3: 12 288); fp32, packed pairs: 2 048 5.25 | 4.90, 4 096 8.3 | 7.4,
  // 16 384 27.0 | 23.5 — from 2 048 (round 3: 8 192))
  if (m <= 6) {
    const int from = for_optimizer ? (elem == 4 ? kOptTwoPerWaveF32From : kOptTwoPerWaveF64From)
                                   : (elem == 4 ? kTwoPerWaveF32From : kTwoPerWaveF64From);
    p.spl = pinned_spl ? pinned_spl : (B >= from ? 6 : 3);
  }
  else if (m <= 12 && !for_optimizer && pinned_spl != 6 &&
           (pinned_spl == 3 || B <= (elem == 4 ? kTwoWavesUpTo / 2 : kTwoWavesUpTo))) {
    // 7 .. 12 segments, a batch that leaves SIMDs idle with one wavefront per trajectory: two wavefronts per
    // trajectory at ten lanes per segment (measured on one box, 12 segments, fp64: B = 1 3.6 us against 5.8 on one
    // wavefront, 256: 4.1 / 6.2, 1 024: 6.2 / 7.0, 1 280: 9.1 / 9.4; fp32, whose one-wavefront body runs packed
    // pairs: 512: 4.9 / 7.1, 768: 5.1 / 4.9)
    p.spl = 3;
    p.nw = 2;
  } else if (pinned_spl == 3) return false;   // ten lanes per segment: six segments fill a wavefront, twelve fill two
  else p.spl = 6;
  p.is_long = m > 12;
  p.nt = (p.spl == 6 && 2 * m <= 12) ? 2 : 1;
  // (the optimizer's state and tile are fp64 whatever precision its evaluations run in)
  if (gtop_wave_lds_bytes(p, m, for_optimizer ? sizeof(double) : elem, for_optimizer) > 160u * 1024u) return false;   // ~200 segments
  *plan = p;
  return true;
}

// The launch rule of the moving-obstacle bodies (fp64): the static rule restricted to the geometries that have one.
// Auto: up to 6 segments ten lanes per segment, from the static rule's own switch point five lanes per segment with two
// trajectories per wavefront (the optimizer loop: one); 7 .. 12 segments five lanes per segment; past 12 the chunked
// body.  Pinned 3 / 6 as in the static rule, except that 3 with 7 .. 12 segments (two wavefronts per trajectory) and
// 10 / 30 (three lanes, one lane per segment) have no moving-term body: false.
bool gtop_eval_plan_moving(int B, int m, int pinned_spl, bool for_optimizer, GtopEvalPlan *plan) {
  if (pinned_spl == 10 || pinned_spl == 30) return false;
  int pin = pinned_spl;
  if (pin == 0)
    pin = m <= 6 ? (B >= (for_optimizer ? kOptTwoPerWaveF64From : kTwoPerWaveF64From) ? 6 : 3) : 6;
  GtopEvalPlan p{};
  if (!gtop_eval_plan(B, m, sizeof(double), pin, for_optimizer, &p)) return false;
  if (for_optimizer && p.nt == 2 && !gtop_eval_plan(B, m, sizeof(double), 3, true, &p)) return false;
  if (p.nw != 1 || (p.spl != 3 && p.spl != 6)) return false;
  *plan = p;
  return true;
}
