/*
 * gtop_oracle.c — CPU restatement of GTOP's cost/gradient callback.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under oracle/ is product code: only
 * tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load
 * this library, and only as the checker / the reported CPU baseline.  The
 * product path (grad_traj_optimization_amd/) never links or calls it.
 *
 * PARITY UNPINNED: the reference ships no tests, golden vectors or fixtures
 * for this path and cannot be compiled in this image (it needs Eigen3, ROS
 * and NLopt headers, none present).  This file follows the cited reference
 * lines statement by statement (dense L/R from an LU inverse, pow(), the
 * float round-trip of pos/vel, the extra `cd` factor, +1e-3/+1e-5 offsets);
 * it is cross-checked against an independently written numpy twin
 * (oracle/np_twin.py) and against structural known answers derivable from
 * the reference source (tests/test_oracle.py).
 *
 * All citations are file:line into /root/reference/.
 * Matrices are dense row-major doubles.
 */
#define _POSIX_C_SOURCE 200809L
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#include "gtop_oracle.h"

/* ------------------------------------------------------------------ */
/* dense helpers                                                      */
/* ------------------------------------------------------------------ */

static double *dalloc(size_t n) {
  double *p = (double *)calloc(n ? n : 1, sizeof(double));
  return p;
}

/* C(r×c) = A(r×k) · B(k×c) */
static void matmul(int r, int k, int c, const double *A, const double *B,
                   double *C) {
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < c; ++j) {
      double s = 0.0;
      for (int p = 0; p < k; ++p) s += A[i * k + p] * B[p * c + j];
      C[i * c + j] = s;
    }
}

static void transpose(int r, int c, const double *A, double *At) {
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < c; ++j) At[j * r + i] = A[i * c + j];
}

/* inverse by LU with partial pivoting — what Eigen's MatrixXd::inverse()
 * (PartialPivLU) does for dynamic sizes (qp_generator.cpp:390-393). */
static int lu_inverse(int n, const double *Ain, double *inv) {
  double *a = dalloc((size_t)n * n);
  int *piv = (int *)malloc(sizeof(int) * (size_t)n);
  memcpy(a, Ain, sizeof(double) * (size_t)n * n);
  for (int i = 0; i < n; ++i) piv[i] = i;
  for (int k = 0; k < n; ++k) {
    int p = k;
    double best = fabs(a[k * n + k]);
    for (int i = k + 1; i < n; ++i)
      if (fabs(a[i * n + k]) > best) {
        best = fabs(a[i * n + k]);
        p = i;
      }
    if (best == 0.0) {
      free(a);
      free(piv);
      return -1;
    }
    if (p != k) {
      for (int j = 0; j < n; ++j) {
        double t = a[k * n + j];
        a[k * n + j] = a[p * n + j];
        a[p * n + j] = t;
      }
      int t = piv[k];
      piv[k] = piv[p];
      piv[p] = t;
    }
    for (int i = k + 1; i < n; ++i) {
      a[i * n + k] /= a[k * n + k];
      double l = a[i * n + k];
      if (l != 0.0)
        for (int j = k + 1; j < n; ++j) a[i * n + j] -= l * a[k * n + j];
    }
  }
  /* solve A X = I column by column: L U x = P e_c */
  double *y = dalloc((size_t)n);
  for (int c = 0; c < n; ++c) {
    for (int i = 0; i < n; ++i) {
      double s = (piv[i] == c) ? 1.0 : 0.0;
      for (int j = 0; j < i; ++j) s -= a[i * n + j] * y[j];
      y[i] = s;
    }
    for (int i = n - 1; i >= 0; --i) {
      double s = y[i];
      for (int j = i + 1; j < n; ++j) s -= a[i * n + j] * inv[j * n + c];
      inv[i * n + c] = s / a[i * n + i];
    }
  }
  free(y);
  free(a);
  free(piv);
  return 0;
}

static int factorial(int x) { /* qp_generator.cpp:173-179 */
  int fac = 1;
  for (int i = x; i > 0; i--) fac = fac * i;
  return fac;
}

/* ------------------------------------------------------------------ */
/* setup side: segment times, generator matrices, initial Df/Dp       */
/* ------------------------------------------------------------------ */

/* grad_traj_optimizer.cpp:73-81.  Note `i == segment_time.size()` is never
 * true inside the loop, so only the FIRST segment receives init_time. */
void oracle_segment_time(int npts, const double *path, double mean_v,
                         double init_time, double *T) {
  int m = npts - 1;
  for (int i = 0; i < m; ++i) {
    double dx = path[3 * i + 0] - path[3 * (i + 1) + 0];
    double dy = path[3 * i + 1] - path[3 * (i + 1) + 1];
    double dz = path[3 * i + 2] - path[3 * (i + 1) + 2];
    double len = sqrt(dx * dx + dy * dy + dz * dz);
    if (i == 0 || i == m) {
      T[i] = len / mean_v + init_time;
    } else {
      T[i] = len / mean_v;
    }
  }
}

/* Mapping matrix A (qp_generator.cpp:181-197), jerk Hessian Q (:223-236),
 * selection Ct (:357-387), L = A^-1 Ct (:390),
 * R = C A^-T Q A^-1 Ct (:392-393).  Sizes: A,Q 6m×6m; Ct,L 6m×(3m+3);
 * R (3m+3)². Any output pointer may be NULL.  Returns 0, or -1 if m < 2
 * (StackOptiDep writes out of bounds for m == 1) or A is singular. */
int oracle_generator(int m, const double *T, double *A_out, double *Q_out,
                     double *Ct_out, double *L_out, double *R_out) {
  if (m < 2) return -1;
  int n6 = 6 * m, nd = 3 * m + 3;
  double *A = dalloc((size_t)n6 * n6), *Q = dalloc((size_t)n6 * n6);
  double *Ct = dalloc((size_t)n6 * nd);
  for (int k = 0; k < m; k++) {
    for (int i = 0; i < 3; i++) {
      A[(k * 6 + 2 * i) * n6 + k * 6 + i] = factorial(i);
      for (int j = i; j < 6; j++)
        A[(k * 6 + 2 * i + 1) * n6 + k * 6 + j] =
            factorial(j) / factorial(j - i) * pow(T[k], j - i);
    }
  }
  for (int k = 0; k < m; k++)
    for (int i = 3; i < 6; i++)
      for (int j = 3; j < 6; j++)
        Q[(k * 6 + i) * n6 + k * 6 + j] =
            i * (i - 1) * (i - 2) * j * (j - 1) * (j - 2) / (i + j - 5) *
            pow(T[k], (i + j - 5));

#define CT(r, c) Ct[(r) * nd + (c)]
  CT(0, 0) = 1;
  CT(2, 1) = 1;
  CT(4, 2) = 1;
  CT(1, 6) = 1;
  CT(3, 7) = 1;
  CT(5, 8) = 1;
  CT(6 * (m - 1) + 0, 3 * m + 0) = 1;
  CT(6 * (m - 1) + 2, 3 * m + 1) = 1;
  CT(6 * (m - 1) + 4, 3 * m + 2) = 1;
  CT(6 * (m - 1) + 1, 3) = 1;
  CT(6 * (m - 1) + 3, 4) = 1;
  CT(6 * (m - 1) + 5, 5) = 1;
  for (int j = 2; j < m; j++) {
    CT(6 * (j - 1) + 0, 6 + 3 * (j - 2) + 0) = 1;
    CT(6 * (j - 1) + 1, 6 + 3 * (j - 1) + 0) = 1;
    CT(6 * (j - 1) + 2, 6 + 3 * (j - 2) + 1) = 1;
    CT(6 * (j - 1) + 3, 6 + 3 * (j - 1) + 1) = 1;
    CT(6 * (j - 1) + 4, 6 + 3 * (j - 2) + 2) = 1;
    CT(6 * (j - 1) + 5, 6 + 3 * (j - 1) + 2) = 1;
  }
#undef CT

  double *Ainv = dalloc((size_t)n6 * n6);
  if (lu_inverse(n6, A, Ainv) != 0) {
    free(A);
    free(Q);
    free(Ct);
    free(Ainv);
    return -1;
  }
  double *L = dalloc((size_t)n6 * nd);
  matmul(n6, n6, nd, Ainv, Ct, L);

  /* R = ((( C · B^T ) · Q ) · A^-1 ) · Ct, left to right */
  double *C = dalloc((size_t)nd * n6), *Bt = dalloc((size_t)n6 * n6);
  transpose(n6, nd, Ct, C);
  transpose(n6, n6, Ainv, Bt);
  double *t1 = dalloc((size_t)nd * n6), *t2 = dalloc((size_t)nd * n6);
  matmul(nd, n6, n6, C, Bt, t1);
  matmul(nd, n6, n6, t1, Q, t2);
  matmul(nd, n6, n6, t2, Ainv, t1);
  double *R = dalloc((size_t)nd * nd);
  matmul(nd, n6, nd, t1, Ct, R);

  if (A_out) memcpy(A_out, A, sizeof(double) * (size_t)n6 * n6);
  if (Q_out) memcpy(Q_out, Q, sizeof(double) * (size_t)n6 * n6);
  if (Ct_out) memcpy(Ct_out, Ct, sizeof(double) * (size_t)n6 * nd);
  if (L_out) memcpy(L_out, L, sizeof(double) * (size_t)n6 * nd);
  if (R_out) memcpy(R_out, R, sizeof(double) * (size_t)nd * nd);
  free(A);
  free(Q);
  free(Ct);
  free(Ainv);
  free(L);
  free(C);
  free(Bt);
  free(t1);
  free(t2);
  free(R);
  return 0;
}

/* Straight-line initial derivatives (type == 2 branch of PolyQPGeneration,
 * qp_generator.cpp:199-221, then getInitialD :407-451).
 * Df 3×6 = [p_start, startVel, startAcc, p_end, 0, 0] per axis;
 * Dp 3×(3m-3): interior waypoint positions, vel = acc = 0. */
void oracle_initial_d(int npts, const double *path, const double *vel,
                      const double *acc, double *Df, double *Dp) {
  int m = npts - 1, ndp = 3 * m - 3, n6 = 6 * m;
  double *D[3];
  for (int a = 0; a < 3; ++a) D[a] = dalloc((size_t)n6);
  for (int k = 1; k < m + 1; k++) {
    for (int a = 0; a < 3; ++a) {
      D[a][(k - 1) * 6] = path[3 * (k - 1) + a];
      D[a][(k - 1) * 6 + 1] = path[3 * k + a];
      if (k == 1) {
        D[a][(k - 1) * 6 + 2] = vel[a];
        D[a][(k - 1) * 6 + 4] = acc[a];
      }
    }
  }
  for (int a = 0; a < 3; ++a) {
    for (int j = 0; j < 6; ++j) Df[a * 6 + j] = 0.0;
    Df[a * 6 + 0] = D[a][0];
    Df[a * 6 + 3] = D[a][n6 - 5];
    Df[a * 6 + 1] = vel[a];
    Df[a * 6 + 2] = acc[a];
    for (int k = 1; k < m; k++)
      for (int i = 0; i < 3; i++)
        Dp[a * ndp + (k - 1) * 3 + i] = D[a][(k - 1) * 6 + 2 * i + 1];
  }
  for (int a = 0; a < 3; ++a) free(D[a]);
}

/* ------------------------------------------------------------------ */
/* distance field                                                     */
/* ------------------------------------------------------------------ */

/* sdf_map.cpp:3-24 (grid passed in directly) */
void oracle_sdf_init(oracle_sdf *S, const double origin[3], double resolution,
                     const int grid[3], double *distance_buffer) {
  for (int i = 0; i < 3; ++i) {
    S->origin[i] = origin[i];
    S->grid[i] = grid[i];
    S->min_range[i] = origin[i];
    S->max_range[i] = origin[i] + grid[i] * resolution;
  }
  S->resolution = resolution;
  S->resolution_inv = 1 / resolution;
  S->dist = distance_buffer;
}

/* as sdf_map.cpp:3-24 computes it: map_size given, grid = ceil(size/res),
 * max_range = origin + map_size */
void oracle_sdf_init_size(oracle_sdf *S, const double origin[3],
                          double resolution, const double map_size[3],
                          int grid_out[3]) {
  for (int i = 0; i < 3; ++i) {
    S->origin[i] = origin[i];
    S->grid[i] = (int)ceil(map_size[i] / resolution);
    grid_out[i] = S->grid[i];
    S->min_range[i] = origin[i];
    S->max_range[i] = origin[i] + map_size[i];
  }
  S->resolution = resolution;
  S->resolution_inv = 1 / resolution;
  S->dist = NULL;
}

static int sdf_in_map(const oracle_sdf *S, const double pos[3]) {
  /* sdf_map.cpp:55-69 */
  if (pos[0] < S->min_range[0] + 1e-4 || pos[1] < S->min_range[1] + 1e-4 ||
      pos[2] < S->min_range[2] + 1e-4)
    return 0;
  if (pos[0] > S->max_range[0] - 1e-4 || pos[1] > S->max_range[1] - 1e-4 ||
      pos[2] > S->max_range[2] - 1e-4)
    return 0;
  return 1;
}

static void sdf_pos_to_index(const oracle_sdf *S, const double pos[3],
                             int id[3]) {
  /* sdf_map.cpp:71-74 */
  for (int i = 0; i < 3; ++i)
    id[i] = (int)floor((pos[i] - S->origin[i]) * S->resolution_inv);
}

static double sdf_get_distance(const oracle_sdf *S, int x, int y, int z) {
  /* sdf_map.cpp:166-174: per-axis index clamp */
  int gx = S->grid[0], gy = S->grid[1], gz = S->grid[2];
  x = x < gx - 1 ? x : gx - 1;
  x = x > 0 ? x : 0;
  y = y < gy - 1 ? y : gy - 1;
  y = y > 0 ? y : 0;
  z = z < gz - 1 ? z : gz - 1;
  z = z > 0 ? z : 0;
  return S->dist[(size_t)x * gy * gz + (size_t)y * gz + z];
}

/* sdf_map.cpp:185-242.  Out of map: returns -1 and (convention, SURVEY
 * A.4 Q4: the reference leaves grad uninitialised) grad = 0. */
double oracle_sdf_query(const oracle_sdf *S, const double pos[3],
                        double grad[3]) {
  if (!sdf_in_map(S, pos)) {
    grad[0] = grad[1] = grad[2] = 0.0;
    return -1;
  }
  double res = S->resolution, rinv = S->resolution_inv;
  double pos_m[3], idx_pos[3], diff[3];
  int idx[3];
  for (int i = 0; i < 3; ++i) pos_m[i] = pos[i] - 0.5 * res * 1.0;
  sdf_pos_to_index(S, pos_m, idx);
  for (int i = 0; i < 3; ++i) /* sdf_map.cpp:76-78 */
    idx_pos[i] = (idx[i] + 0.5) * res + S->origin[i];
  for (int i = 0; i < 3; ++i) diff[i] = (pos[i] - idx_pos[i]) * rinv;

  double values[2][2][2];
  for (int x = 0; x < 2; x++)
    for (int y = 0; y < 2; y++)
      for (int z = 0; z < 2; z++)
        values[x][y][z] = sdf_get_distance(S, idx[0] + x, idx[1] + y, idx[2] + z);

  double v00 = (1 - diff[0]) * values[0][0][0] + diff[0] * values[1][0][0];
  double v01 = (1 - diff[0]) * values[0][0][1] + diff[0] * values[1][0][1];
  double v10 = (1 - diff[0]) * values[0][1][0] + diff[0] * values[1][1][0];
  double v11 = (1 - diff[0]) * values[0][1][1] + diff[0] * values[1][1][1];
  double v0 = (1 - diff[1]) * v00 + diff[1] * v10;
  double v1 = (1 - diff[1]) * v01 + diff[1] * v11;
  double dist = (1 - diff[2]) * v0 + diff[2] * v1;

  grad[2] = (v1 - v0) * rinv;
  grad[1] = ((1 - diff[2]) * (v10 - v00) + diff[2] * (v11 - v01)) * rinv;
  grad[0] = (1 - diff[2]) * (1 - diff[1]) * (values[1][0][0] - values[0][0][0]);
  grad[0] += (1 - diff[2]) * diff[1] * (values[1][1][0] - values[0][1][0]);
  grad[0] += diff[2] * (1 - diff[1]) * (values[1][0][1] - values[0][0][1]);
  grad[0] += diff[2] * diff[1] * (values[1][1][1] - values[0][1][1]);
  grad[0] *= rinv;
  return dist;
}

/* Rounding-error magnitudes of oracle_sdf_query at the same position (see oracle_cost_grad_mag): *dmag bounds the
 * value's arithmetic, gmag[k] the gradient's — corner values by magnitude, every difference of two corners as
 * (|v1| + |v0|) (fp32 fields round the corners themselves), and the weights' own absolute error,
 * (|pos| + |idx_pos|) / res + 1, times the value's (gradient's) exact sensitivity to that weight.
 * margins: [0] distance of the cell coordinate (pos - res/2 - origin) / res to an integer (the floor of
 * sdf_map.cpp:201-204), [1] distance of pos to the in-map bounds (:55-69); both relative to their magnitudes. */
static void sdf_query_mag_v(const oracle_sdf *S, const double pos[3], const double *vin, const double *vmin,
                            double *dmag, double gmag[3], double margins[2], double dgdp[3][3]) {
  for (int k = 0; k < 3; ++k) dgdp[k][0] = dgdp[k][1] = dgdp[k][2] = 0;
  double mm = INFINITY;
  for (int i = 0; i < 3; ++i) {
    double lo = S->min_range[i] + 1e-4, hi = S->max_range[i] - 1e-4;
    double sc = fabs(pos[i]) + fabs(S->min_range[i]) + fabs(S->max_range[i]) + 1e-4;
    mm = fmin(mm, fmin(fabs(pos[i] - lo), fabs(pos[i] - hi)) / sc);
  }
  margins[1] = mm;
  if (!sdf_in_map(S, pos)) {
    *dmag = 1.0;
    gmag[0] = gmag[1] = gmag[2] = 0.0;
    margins[0] = INFINITY;
    return;
  }
  double res = S->resolution, rinv = S->resolution_inv;
  double diff[3], wm[3];
  int idx[3];
  double cm = INFINITY;
  for (int i = 0; i < 3; ++i) {
    double u = ((pos[i] - 0.5 * res) - S->origin[i]) * rinv;
    idx[i] = (int)floor(u);
    cm = fmin(cm, fabs(u - nearbyint(u)) / ((fabs(pos[i]) + fabs(S->origin[i]) + res) * rinv));
    double ip = (idx[i] + 0.5) * res + S->origin[i];
    diff[i] = (pos[i] - ip) * rinv;
    wm[i] = (fabs(pos[i]) + fabs(ip)) * rinv + 1.0;
  }
  margins[0] = cm;
  double v[8], vm[8]; /* v[x*4 + y*2 + z]; vm: the corner's own rounding-error magnitude (|v| for a stored value) */
  for (int c = 0; c < 8; c++) {
    v[c] = vin ? vin[c] : sdf_get_distance(S, idx[0] + (c >> 2), idx[1] + ((c >> 1) & 1), idx[2] + (c & 1));
    vm[c] = vmin ? vmin[c] : fabs(v[c]);
  }
  double w[3][2];
  for (int i = 0; i < 3; ++i) {
    w[i][0] = fabs(1 - diff[i]);
    w[i][1] = fabs(diff[i]);
  }
  static const int bit[3] = {4, 2, 1};
  double val = 0, d[3] = {0, 0, 0}, ds[3] = {0, 0, 0}, dd[3][3] = {{0}};
  for (int c = 0; c < 8; c++) {
    const int b[3] = {c >> 2, (c >> 1) & 1, c & 1};
    val += w[0][b[0]] * w[1][b[1]] * w[2][b[2]] * vm[c];
    for (int k = 0; k < 3; ++k) {
      if (b[k]) continue;
      const int o1 = (k + 1) % 3, o2 = (k + 2) % 3;
      const double wo = w[o1][b[o1]] * w[o2][b[o2]];
      d[k] += wo * (vm[c + bit[k]] + vm[c]);            /* the difference's magnitude */
      ds[k] += wo * fabs(v[c + bit[k]] - v[c]);         /* the value's sensitivity to weight k */
      for (int j = 0; j < 3; ++j) {                      /* the k-gradient's sensitivity to weight j */
        if (j == k || b[j]) continue;
        const int l = 3 - j - k;
        dd[k][j] += w[l][b[l]] * fabs((v[c + bit[k] + bit[j]] - v[c + bit[j]]) - (v[c + bit[k]] - v[c]));
      }
    }
  }
  *dmag = val + wm[0] * ds[0] + wm[1] * ds[1] + wm[2] * ds[2];
  for (int k = 0; k < 3; ++k) {
    double e = d[k];
    for (int j = 0; j < 3; ++j)
      if (j != k) {
        e += wm[j] * dd[k][j];
        dgdp[k][j] = dd[k][j] * rinv * rinv;   /* |d grad_k / d pos_j| */
      }
    gmag[k] = e * rinv;
  }
}

/* pre-rounding doubles closer than FLIP_TAU * magnitude to a float rounding boundary may round either way in an
 * implementation whose coefficients round differently (2^9 u64: the sample polynomial's ~25 u plus the 150 u of
 * the sample times, see tests/test_gpu_entrywise.py) */
#define FLIP_TAU 0x1p-44

/* distance of a double to the nearest rounding boundary of (float), relative to `mag`.  With `noise` a value whose
 * float spacing is below 2^-42 mag (a velocity that cancels to nearly nothing) is no decision: either rounding moves
 * it by less than its own arithmetic's error at any kappa64 >= 2^11, which the magnitudes already carry (they take
 * such values by their magnitude, not their size). */
static double float_margin(double pre, double mag, int noise) {
  float f = (float)pre;
  if (!isfinite(f) || !(mag > 0)) return INFINITY;
  double up = nextafterf(f, INFINITY), dn = nextafterf(f, -INFINITY);
  if (noise && up - (double)f <= 0x1p-42 * mag) return INFINITY;
  double hi = 0.5 * ((double)f + up), lo = 0.5 * ((double)f + dn);
  return fmin(fabs(pre - hi), fabs(pre - lo)) / mag;
}

/* EDTEnvironment::distToBox / minDistToAllBox, src/edt_environment.cpp:26-73.
 * A box is {p0, vel, scale}: its centre at `time` is the constant-velocity
 * prediction p0 + vel*time (ObjPrediction::evaluateConstVel,
 * include/grad_traj_optimization/obj_predictor.h:57-66). */
static double edt_min_dist_to_boxes(int nbox, const double *p0, const double *vel, const double *scale,
                                    const double pt[3], double time) {
  double dist = 10000000.0; /* :64 */
  for (int b = 0; b < nbox; ++b) {
    double d2 = 0.0;
    for (int i = 0; i < 3; ++i) {
      double c = p0[3 * b + i] + vel[3 * b + i] * time;
      double bmax = c + 0.5 * scale[3 * b + i], bmin = c - 0.5 * scale[3 * b + i]; /* :31-32 */
      double di = (pt[i] >= bmin && pt[i] <= bmax) ? 0.0 : fmin(fabs(pt[i] - bmin), fabs(pt[i] - bmax)); /* :36-40 */
      d2 += di * di;
    }
    double di = sqrt(d2); /* dist.norm(), :42 */
    if (di < dist) dist = di;
  }
  return dist;
}

/* EDTEnvironment::evaluateCoarseEDT, src/edt_environment.cpp:124-136: the distance of the voxel that holds
 * `pos` (SDFMap::getDistance(Vector3d), src/sdf_map.cpp:155-164: -1 outside the map), and with time >= 0 its
 * minimum with the distance from `pos` itself to the nearest moving box.  No interpolation, no gradient. */
double oracle_edt_coarse(const oracle_sdf *S, int nbox, const double *box_p0, const double *box_vel,
                         const double *box_scale, const double pos[3], double time) {
  double d1 = -1.0;
  if (sdf_in_map(S, pos)) {
    int id[3];
    sdf_pos_to_index(S, pos, id);
    d1 = sdf_get_distance(S, id[0], id[1], id[2]);
  }
  if (time < 0.0) return d1;
  double d2 = edt_min_dist_to_boxes(nbox, box_p0, box_vel, box_scale, pos, time);
  return d1 < d2 ? d1 : d2;
}

/* EDTEnvironment::evaluateEDTWithGrad, src/edt_environment.cpp:75-122: the
 * trilinear value/gradient over corner values min(static distance, distance
 * to the nearest moving box at `time`); time < 0 means static only (:91-94).
 * That file is not part of the reference's build and calls an SDFMap API the
 * in-tree class does not have (getInterpolationData); the interpolation data
 * here are the in-tree ones (sdf_map.cpp:201-219: base index, diff, per-axis
 * clamped corner loads), a corner's position is the centre of its (unclamped)
 * voxel, and a query outside the map returns -1 with a zero gradient as
 * oracle_sdf_query does.  PARITY UNPINNED (no reference output exists). */
double oracle_edt_query(const oracle_sdf *S, int nbox, const double *box_p0, const double *box_vel,
                        const double *box_scale, const double pos[3], double time, double grad[3]) {
  if (!sdf_in_map(S, pos)) {
    grad[0] = grad[1] = grad[2] = 0.0;
    return -1;
  }
  double res = S->resolution, rinv = S->resolution_inv;
  double pos_m[3], idx_pos[3], diff[3];
  int idx[3];
  for (int i = 0; i < 3; ++i) pos_m[i] = pos[i] - 0.5 * res * 1.0;
  sdf_pos_to_index(S, pos_m, idx);
  for (int i = 0; i < 3; ++i) idx_pos[i] = (idx[i] + 0.5) * res + S->origin[i];
  for (int i = 0; i < 3; ++i) diff[i] = (pos[i] - idx_pos[i]) * rinv;

  double values[2][2][2];
  for (int x = 0; x < 2; x++)
    for (int y = 0; y < 2; y++)
      for (int z = 0; z < 2; z++) {
        double d1 = sdf_get_distance(S, idx[0] + x, idx[1] + y, idx[2] + z);
        if (time < 0.0) { /* :91-94 */
          values[x][y][z] = d1;
        } else {
          double pt[3] = {(idx[0] + x + 0.5) * res + S->origin[0], (idx[1] + y + 0.5) * res + S->origin[1],
                          (idx[2] + z + 0.5) * res + S->origin[2]};
          double d2 = edt_min_dist_to_boxes(nbox, box_p0, box_vel, box_scale, pt, time);
          values[x][y][z] = d1 < d2 ? d1 : d2; /* :98 */
        }
      }

  double v00 = (1 - diff[0]) * values[0][0][0] + diff[0] * values[1][0][0]; /* :104-112 */
  double v01 = (1 - diff[0]) * values[0][0][1] + diff[0] * values[1][0][1];
  double v10 = (1 - diff[0]) * values[0][1][0] + diff[0] * values[1][1][0];
  double v11 = (1 - diff[0]) * values[0][1][1] + diff[0] * values[1][1][1];
  double v0 = (1 - diff[1]) * v00 + diff[1] * v10;
  double v1 = (1 - diff[1]) * v01 + diff[1] * v11;
  double dist = (1 - diff[2]) * v0 + diff[2] * v1;

  grad[2] = (v1 - v0) * rinv; /* :114-121 */
  grad[1] = ((1 - diff[2]) * (v10 - v00) + diff[2] * (v11 - v01)) * rinv;
  grad[0] = (1 - diff[2]) * (1 - diff[1]) * (values[1][0][0] - values[0][0][0]);
  grad[0] += (1 - diff[2]) * diff[1] * (values[1][1][0] - values[0][1][0]);
  grad[0] += diff[2] * (1 - diff[1]) * (values[1][0][1] - values[0][0][1]);
  grad[0] += diff[2] * diff[1] * (values[1][1][1] - values[0][1][1]);
  grad[0] *= rinv;
  return dist;
}

/* Centre of box b on axis i at `tau` for either list kind (oracle_ext, gtop_oracle.h) and its rounding-error
 * magnitude.  Constant velocity: p0 + vel*tau (obj_predictor.h:57-66), magnitude |p0| + |vel| |tau|.  Polynomial
 * (include/gtop.h): tc = fmin(fmax(tau, t1), t2), then Horner in explicit fma; magnitude sum |c_j| |tc|^j.  The
 * sample time itself differs between implementations (t += dt against 1e-3 + i dt: a few tens of u of t <= tau, and
 * one rounding of the sum): its effect on the centre is the derivative's magnitude times |tau| — already in
 * |vel| |tau| for a constant velocity, sum j |c_j| |tc|^(j-1) |tau| for a polynomial (kept when the clamp binds: the
 * clamp is continuous, and a tau within rounding of t1 / t2 may clamp in one implementation and not in the other). */
static double ext_box_centre(const oracle_ext *E, int b, int i, double tau, double *cmag) {
  if (!E->poly) {
    *cmag = fabs(E->p0[3 * b + i]) + fabs(E->vel[3 * b + i]) * fabs(tau);
    return E->p0[3 * b + i] + E->vel[3 * b + i] * tau;
  }
  double tc = tau;
  if (E->t_range) tc = fmin(fmax(tau, E->t_range[2 * b]), E->t_range[2 * b + 1]);
  const double *c = E->coef + 18 * b + 6 * i;
  double r = c[5];
  for (int j = 4; j >= 0; --j) r = fma(r, tc, c[j]);
  double hm = 0, dm = 0, pw = 1, pw1 = 0;
  const double at = fabs(tc);
  for (int j = 0; j < 6; ++j) {
    hm += fabs(c[j]) * pw;
    dm += j * fabs(c[j]) * pw1;
    pw1 = pw;
    pw *= at;
  }
  *cmag = hm + dm * fabs(tau);
  return r;
}

/* distToBox (src/edt_environment.cpp:26-45) of one box at `pt` with its rounding-error magnitude.  Per axis the
 * face coordinates c +- scale/2 and the point carry em_i = ptm_i + cmag_i + |scale_i|/2; the slab distance d_i is
 * continuous in them (the inside test meets the face distance at 0), so it moves by at most em_i u — and not at all
 * where the point is inside the slab by more than that.  ||d + e|| - ||d|| <= ||e||: the norm's error is
 * sqrt(sum e_i^2), plus its own rounding, d. */
static double ext_box_dist(const oracle_ext *E, int b, const double pt[3], const double ptm[3], double tau,
                           double *mag2) {
  double d2 = 0.0, e2 = 0.0;
  for (int i = 0; i < 3; ++i) {
    double cmag;
    const double c = ext_box_centre(E, b, i, tau, &cmag);
    const double h = 0.5 * E->scale[3 * b + i];
    const double bmax = c + h, bmin = c - h; /* :31-32 */
    const int inside = pt[i] >= bmin && pt[i] <= bmax;
    const double di = inside ? 0.0 : fmin(fabs(pt[i] - bmin), fabs(pt[i] - bmax)); /* :36-40 */
    const double em = ptm[i] + cmag + fabs(h);
    const double depth = fmin(pt[i] - bmin, bmax - pt[i]);
    const double ei = (!inside || depth < 0x1p-40 * em) ? em : 0.0;
    d2 += di * di;
    e2 += ei * ei;
  }
  const double d = sqrt(d2); /* dist.norm(), :42 */
  *mag2 = d + sqrt(e2);
  return d;
}

/* oracle_edt_query's arithmetic with the box list of an oracle_ext; also the 8 corner values v[x*4 + y*2 + z] and
 * their magnitudes vm[] for sdf_query_mag_v, and *lowered = 1 if a box lowered any corner.  The min over boxes and
 * with the static value is continuous, so a corner's magnitude is that of the value taken — and the larger of the
 * two where they lie within 2^-40 of the box distance's magnitude of each other (either may win). */
static double edt_query_ext(const oracle_sdf *S, const oracle_ext *E, const double pos[3], double time, double grad[3],
                            double v[8], double vm[8], int *lowered) {
  *lowered = 0;
  if (!sdf_in_map(S, pos)) {
    grad[0] = grad[1] = grad[2] = 0.0;
    for (int c = 0; c < 8; ++c) v[c] = vm[c] = 0.0;
    return -1;
  }
  double res = S->resolution, rinv = S->resolution_inv;
  double pos_m[3], idx_pos[3], diff[3];
  int idx[3];
  for (int i = 0; i < 3; ++i) pos_m[i] = pos[i] - 0.5 * res * 1.0;
  sdf_pos_to_index(S, pos_m, idx);
  for (int i = 0; i < 3; ++i) idx_pos[i] = (idx[i] + 0.5) * res + S->origin[i];
  for (int i = 0; i < 3; ++i) diff[i] = (pos[i] - idx_pos[i]) * rinv;

  double values[2][2][2];
  for (int x = 0; x < 2; x++)
    for (int y = 0; y < 2; y++)
      for (int z = 0; z < 2; z++) {
        const int o[3] = {x, y, z};
        double d1 = sdf_get_distance(S, idx[0] + x, idx[1] + y, idx[2] + z);
        double val = d1, valm = fabs(d1);
        if (!(time < 0.0)) { /* :91-94 */
          double pt[3], ptm[3];
          for (int i = 0; i < 3; ++i) {
            pt[i] = (idx[i] + o[i] + 0.5) * res + S->origin[i];
            ptm[i] = fabs(idx[i] + o[i] + 0.5) * res + fabs(S->origin[i]);
          }
          double dmin = 10000000.0, dmag = 10000000.0; /* :64 */
          for (int b = 0; b < E->nbox; ++b) {
            double m2;
            const double di = ext_box_dist(E, b, pt, ptm, time, &m2);
            if (di < dmin) dmin = di;
          }
          int first = 1;
          for (int b = 0; b < E->nbox; ++b) { /* the magnitude: the largest among the boxes that can be the nearest */
            double m2;
            const double di = ext_box_dist(E, b, pt, ptm, time, &m2);
            if (di <= dmin + 0x1p-40 * m2 && (first || m2 > dmag)) {
              dmag = m2;
              first = 0;
            }
          }
          const double d2 = dmin;
          val = d1 < d2 ? d1 : d2; /* :98 */
          if (d2 < d1) *lowered = 1;
          if (d2 < d1 - 0x1p-40 * dmag) valm = dmag;
          else if (d2 < d1 + 0x1p-40 * dmag) valm = fmax(dmag, fabs(d1));
        }
        values[x][y][z] = val;
        v[x * 4 + y * 2 + z] = val;
        vm[x * 4 + y * 2 + z] = valm;
      }

  double v00 = (1 - diff[0]) * values[0][0][0] + diff[0] * values[1][0][0]; /* :104-112 */
  double v01 = (1 - diff[0]) * values[0][0][1] + diff[0] * values[1][0][1];
  double v10 = (1 - diff[0]) * values[0][1][0] + diff[0] * values[1][1][0];
  double v11 = (1 - diff[0]) * values[0][1][1] + diff[0] * values[1][1][1];
  double v0 = (1 - diff[1]) * v00 + diff[1] * v10;
  double v1 = (1 - diff[1]) * v01 + diff[1] * v11;
  double dist = (1 - diff[2]) * v0 + diff[2] * v1;

  grad[2] = (v1 - v0) * rinv; /* :114-121 */
  grad[1] = ((1 - diff[2]) * (v10 - v00) + diff[2] * (v11 - v01)) * rinv;
  grad[0] = (1 - diff[2]) * (1 - diff[1]) * (values[1][0][0] - values[0][0][0]);
  grad[0] += (1 - diff[2]) * diff[1] * (values[1][1][0] - values[0][1][0]);
  grad[0] += diff[2] * (1 - diff[1]) * (values[1][0][1] - values[0][0][1]);
  grad[0] += diff[2] * diff[1] * (values[1][1][1] - values[0][1][1]);
  grad[0] *= rinv;
  return dist;
}

/* sdf_map.cpp:80-99: mark the voxel containing pos occupied (if in map). */
int oracle_set_occupancy(const oracle_sdf *S, double *occupancy,
                         const double pos[3], int occ) {
  if (occ != 1 && occ != 0) return -1;
  if (!sdf_in_map(S, pos)) return 0;
  int id[3];
  sdf_pos_to_index(S, pos, id);
  occupancy[(size_t)id[0] * S->grid[1] * S->grid[2] +
            (size_t)id[1] * S->grid[2] + id[2]] = occ;
  return 1;
}

/* sdf_map.cpp:266-308: 1-D lower-envelope squared-distance transform.
 * get/set are expressed through a strided view: f[q*stride]. */
static void fill_esdf(const double *fin, size_t in_stride, double *fout,
                      size_t out_stride, int start, int end, int n,
                      int final_pass, double resolution) {
  int *v = (int *)malloc(sizeof(int) * (size_t)(n > 0 ? n : 1));
  double *z = (double *)malloc(sizeof(double) * (size_t)(n + 1));
  int k = start;
  v[start] = start;
  z[start] = -DBL_MAX;
  z[start + 1] = DBL_MAX;
  for (int q = start + 1; q <= end; q++) {
    k++;
    double s;
    do {
      k--;
      s = ((fin[(size_t)q * in_stride] + q * q) -
           (fin[(size_t)v[k] * in_stride] + v[k] * v[k])) /
          (2 * q - 2 * v[k]);
    } while (s <= z[k]);
    k++;
    v[k] = q;
    z[k] = s;
    z[k + 1] = DBL_MAX;
  }
  k = start;
  for (int q = start; q <= end; q++) {
    while (z[k + 1] < q) k++;
    double val = (q - v[k]) * (q - v[k]) + fin[(size_t)v[k] * in_stride];
    if (final_pass) {
      /* sdf_map.cpp:355-361: min(res*sqrt(val), previous distance) */
      double d = resolution * sqrt(val);
      double old = fout[(size_t)q * out_stride];
      fout[(size_t)q * out_stride] = d < old ? d : old;
    } else {
      fout[(size_t)q * out_stride] = val;
    }
  }
  free(v);
  free(z);
}

/* sdf_map.cpp:310-368 over the full grid (min_vec = 0, max_vec = grid-1).
 * `distance` must hold the previous distances (10000 after a reset,
 * sdf_map.cpp:22,51). */
void oracle_esdf_build(const oracle_sdf *S, const double *occupancy,
                       double *distance) {
  int gx = S->grid[0], gy = S->grid[1], gz = S->grid[2];
  size_t N = (size_t)gx * gy * gz;
  double *tmp0 = (double *)malloc(sizeof(double) * N);
  double *tmp1 = (double *)malloc(sizeof(double) * N);
  double *tmp2 = (double *)malloc(sizeof(double) * N);
  for (size_t i = 0; i < N; ++i) tmp0[i] = occupancy[i] == 1 ? 0 : DBL_MAX;
  for (int x = 0; x < gx; x++)
    for (int y = 0; y < gy; y++) {
      size_t base = (size_t)x * gy * gz + (size_t)y * gz;
      fill_esdf(tmp0 + base, 1, tmp1 + base, 1, 0, gz - 1, gz, 0, 0.0);
    }
  for (int x = 0; x < gx; x++)
    for (int z = 0; z < gz; z++) {
      size_t base = (size_t)x * gy * gz + z;
      fill_esdf(tmp1 + base, (size_t)gz, tmp2 + base, (size_t)gz, 0, gy - 1, gy,
                0, 0.0);
    }
  for (int y = 0; y < gy; y++)
    for (int z = 0; z < gz; z++) {
      size_t base = (size_t)y * gz + z;
      fill_esdf(tmp2 + base, (size_t)gy * gz, distance + base, (size_t)gy * gz,
                0, gx - 1, gx, 1, S->resolution);
    }
  free(tmp0);
  free(tmp1);
  free(tmp2);
}

/* sdf_map.cpp:28-45 / :244-260: the voxel window of (min_pos, max_pos) as resetBuffer(min, max) and setUpdateRange
 * compute it — both clamp the positions to [min_range, max_range], then posToIndex(min_pos) and
 * posToIndex(max_pos - res/2). */
void oracle_window_ids(const oracle_sdf *S, const double min_pos_in[3],
                       const double max_pos_in[3], int min_id[3], int max_id[3]) {
  double min_pos[3], max_pos[3], shifted[3];
  for (int i = 0; i < 3; ++i) {
    min_pos[i] = min_pos_in[i] > S->min_range[i] ? min_pos_in[i] : S->min_range[i];   /* max(min_pos, min_range) */
    max_pos[i] = max_pos_in[i] < S->max_range[i] ? max_pos_in[i] : S->max_range[i];   /* min(max_pos, max_range) */
    shifted[i] = max_pos[i] - S->resolution / 2;
  }
  sdf_pos_to_index(S, min_pos, min_id);
  sdf_pos_to_index(S, shifted, max_id);
}

/* sdf_map.cpp:28-53: resetBuffer(min_pos, max_pos) — occupancy 0 and distance 10000 inside the window only. */
void oracle_reset_window(const oracle_sdf *S, double *occupancy, double *distance,
                         const double min_pos[3], const double max_pos[3]) {
  int lo[3], hi[3];
  oracle_window_ids(S, min_pos, max_pos, lo, hi);
  int gy = S->grid[1], gz = S->grid[2];
  for (int x = lo[0]; x <= hi[0]; ++x)
    for (int y = lo[1]; y <= hi[1]; ++y)
      for (int z = lo[2]; z <= hi[2]; ++z) {
        occupancy[(size_t)x * gy * gz + (size_t)y * gz + z] = 0.0;
        distance[(size_t)x * gy * gz + (size_t)y * gz + z] = 10000;
      }
}

/* sdf_map.cpp:310-368 with the window min_vec .. max_vec that setUpdateRange (:244-264) left behind: the three sweeps
 * run over the window only and see only the window's part of every line; distances outside keep their values, inside
 * they become min(res*sqrt(val), previous) (:355-361).  tmp1 / tmp2 are the object's tmp_buffer1 / tmp_buffer2. */
void oracle_esdf_build_window(const oracle_sdf *S, const double *occupancy,
                              double *distance, const int lo[3], const int hi[3]) {
  int gx = S->grid[0], gy = S->grid[1], gz = S->grid[2];
  size_t N = (size_t)gx * gy * gz;
  double *tmp0 = (double *)malloc(sizeof(double) * N);
  double *tmp1 = (double *)calloc(N, sizeof(double));
  double *tmp2 = (double *)calloc(N, sizeof(double));
  for (size_t i = 0; i < N; ++i) tmp0[i] = occupancy[i] == 1 ? 0 : DBL_MAX;
  int n = gx > gy ? (gx > gz ? gx : gz) : (gy > gz ? gy : gz);
  for (int x = lo[0]; x <= hi[0]; x++)
    for (int y = lo[1]; y <= hi[1]; y++) {
      size_t base = (size_t)x * gy * gz + (size_t)y * gz;
      fill_esdf(tmp0 + base, 1, tmp1 + base, 1, lo[2], hi[2], n, 0, 0.0);
    }
  for (int x = lo[0]; x <= hi[0]; x++)
    for (int z = lo[2]; z <= hi[2]; z++) {
      size_t base = (size_t)x * gy * gz + z;
      fill_esdf(tmp1 + base, (size_t)gz, tmp2 + base, (size_t)gz, lo[1], hi[1], n, 0, 0.0);
    }
  for (int y = lo[1]; y <= hi[1]; y++)
    for (int z = lo[2]; z <= hi[2]; z++) {
      size_t base = (size_t)y * gz + z;
      fill_esdf(tmp2 + base, (size_t)gy * gz, distance + base, (size_t)gy * gz, lo[0], hi[0], n, 1,
                S->resolution);
    }
  free(tmp0);
  free(tmp1);
  free(tmp2);
}

/* ------------------------------------------------------------------ */
/* the hot path                                                       */
/* ------------------------------------------------------------------ */

/* grad_traj_optimizer.cpp:281-432 with :253-279, :451-505, :507-551 and
 * sdf_map.cpp:185-242 underneath.  L: 6m×(3m+3), R: (3m+3)², Df: 3×6,
 * x/grad: 3·num_dp axis-major (:182-187, :428-432).  Returns the cost.
 * With mag != NULL also the rounding-error magnitudes and decision margins of
 * oracle_cost_grad_mag (gtop_oracle.h). */
static double cost_grad_impl(int m, const double *L, const double *R,
                             const double *Df, const double *T,
                             const oracle_params *prm, const oracle_sdf *S,
                             const double *x, double *grad_out, double *mag,
                             const oracle_ext *ext, double t0, int *nlowered) {
  const int cons = ext && ext->mode == 1, boxes = ext && ext->nbox > 0;
  int low_count = 0;
  double seg_start = t0; /* tests/moving_twin.py sample_times: ((t0 + T[0]) + ...) + T[s-1], then + t */
  const int num_df = 6, num_dp = 3 * m - 3, nd = num_df + num_dp, n6 = 6 * m;
  double cost_smooth = 0, cost_colli = 0, cost_vel = 0, cost_acc = 0;
  double *g_smooth = dalloc((size_t)3 * num_dp);
  double *g_colli = dalloc((size_t)3 * num_dp);
  double *g_vel = dalloc((size_t)3 * num_dp);
  double *g_acc = dalloc((size_t)3 * num_dp);
  double *d = dalloc((size_t)3 * nd); /* [df;dp] per axis, :302-323 */
  double *coe = dalloc((size_t)m * 18);
  double *tmp = dalloc((size_t)nd);

  for (int a = 0; a < 3; ++a) {
    for (int j = 0; j < 6; ++j) d[a * nd + j] = Df[a * 6 + j];
    for (int j = 0; j < num_dp; ++j) d[a * nd + 6 + j] = x[j + num_dp * a];
  }

  /* smoothness cost d'Rd (:326-327): (d' R) d */
  for (int a = 0; a < 3; ++a) {
    const double *da = d + a * nd;
    for (int j = 0; j < nd; ++j) {
      double s = 0;
      for (int i = 0; i < nd; ++i) s += da[i] * R[i * nd + j];
      tmp[j] = s;
    }
    double q = 0;
    for (int j = 0; j < nd; ++j) q += tmp[j] * da[j];
    cost_smooth += q;
  }
  /* smoothness gradient 2 Rfp' df + 2 Rpp dp (:330-336);
   * Rfp = R[0:6, 6:], Rpp = R[6:, 6:] (qp_generator.cpp:400-403) */
  for (int a = 0; a < 3; ++a) {
    const double *da = d + a * nd;
    for (int j = 0; j < num_dp; ++j) {
      double s1 = 0, s2 = 0;
      for (int i = 0; i < 6; ++i) s1 += (2 * R[i * nd + 6 + j]) * da[i];
      for (int i = 0; i < num_dp; ++i)
        s2 += (2 * R[(6 + j) * nd + 6 + i]) * da[6 + i];
      g_smooth[a * num_dp + j] = s1 + s2;
    }
  }
  /* coefficients coe = L d (:253-279) */
  for (int a = 0; a < 3; ++a) {
    const double *da = d + a * nd;
    for (int r = 0; r < n6; ++r) {
      double s = 0;
      for (int i = 0; i < nd; ++i) s += L[r * nd + i] * da[i];
      coe[(r / 6) * 18 + 6 * a + (r % 6)] = s;
    }
  }

  /* magnitudes: |c| = |L||d|; smoothness ws·Σ|c|'Q|c| and 2ws|L|'Q|L||d| (the
   * coefficient-space form, Q_s of qp_generator.cpp:226-234) */
  double *cabs = NULL, *gm_s = NULL, *gm_c = NULL, *gm_v = NULL, *gm_a = NULL;
  double cm_s = 0, cm_c = 0, cm_v = 0, cm_a = 0, fl_c = 0, fl_cd = 0;
  double *fl_g = NULL, *fl_gd = NULL;
  double mg_float = INFINITY, mg_cell = INFINITY, mg_map = INFINITY, mg_count = INFINITY;
  if (mag) {
    cabs = dalloc((size_t)m * 18);
    gm_s = dalloc((size_t)3 * num_dp);
    gm_c = dalloc((size_t)3 * num_dp);
    gm_v = dalloc((size_t)3 * num_dp);
    gm_a = dalloc((size_t)3 * num_dp);
    fl_g = dalloc((size_t)3 * num_dp);
    fl_gd = dalloc((size_t)3 * num_dp);
    double *qc = dalloc((size_t)n6);
    for (int a = 0; a < 3; ++a) {
      const double *da = d + a * nd;
      for (int r = 0; r < n6; ++r) {
        double sm = 0;
        for (int i = 0; i < nd; ++i) sm += fabs(L[r * nd + i]) * fabs(da[i]);
        cabs[(r / 6) * 18 + 6 * a + (r % 6)] = sm;
      }
      for (int sg = 0; sg < m; ++sg) {
        const double *cs = cabs + sg * 18 + 6 * a;
        for (int i = 0; i < 6; ++i) {
          double q = 0;
          for (int j = 3; j < 6 && i >= 3; ++j)
            q += (double)(i * (i - 1) * (i - 2) * j * (j - 1) * (j - 2) / (i + j - 5)) * pow(T[sg], i + j - 5) * cs[j];
          qc[sg * 6 + i] = q;
          cm_s += cs[i] * q;
        }
      }
      for (int j = 0; j < num_dp; ++j) {
        double sm = 0;
        for (int r = 0; r < n6; ++r) sm += fabs(L[r * nd + 6 + j]) * qc[r];
        gm_s[a * num_dp + j] = 2 * sm;
      }
    }
    free(qc);
  }

  double *Ldp = dalloc((size_t)6 * num_dp);
  for (int s = 0; s < m; s++) {
    if (fabs(prm->wc) < 1e-4) break; /* :346 */
    for (int r = 0; r < 6; ++r)      /* :348 */
      for (int c = 0; c < num_dp; ++c)
        Ldp[r * num_dp + c] = L[(6 * s + r) * nd + 6 + c];
    double dt = T[s] / 30.0; /* :351 */
    const double *c = coe + s * 18;
    double t = 1e-3, t_in = 0;
    for (; t < T[s]; t += dt) { /* :353 */
      t_in = t;
      const double tau = seg_start + t;
      /* :451-468, :471-488 — note the float locals */
      double pos[3], vel[3], acc[3], pmag[3], vmag[3], amag[3], pflip[3] = {0, 0, 0}, vflip[3] = {0, 0, 0};
      int vsign[3] = {0, 0, 0}, asign[3] = {0, 0, 0}; /* mode 1: sgn() of a value within FLIP_TAU of its magnitude from 0 */
      for (int a = 0; a < 3; ++a) {
        const double *q = c + 6 * a;
        double pd = q[0] + q[1] * t + q[2] * pow(t, 2) + q[3] * pow(t, 3) +
                    q[4] * pow(t, 4) + q[5] * pow(t, 5);
        double vd = q[1] + 2 * q[2] * pow(t, 1) + 3 * q[3] * pow(t, 2) +
                    4 * q[4] * pow(t, 3) + 5 * q[5] * pow(t, 4);
        float p = pd;
        float v = vd;
        pos[a] = p;
        vel[a] = v;
        if (mag) {
          const double *qa = cabs + s * 18 + 6 * a;
          pmag[a] = vmag[a] = amag[a] = 0;
          for (int i = 0; i < 6; ++i) {
            pmag[a] += qa[i] * pow(t, i);
            if (i >= 1) vmag[a] += i * qa[i] * pow(t, i - 1);
            if (i >= 2) amag[a] += i * (i - 1) * qa[i] * pow(t, i - 2);
          }
          const double mp_ = float_margin(pd, pmag[a], 0), mv_ = float_margin(vd, vmag[a], 1);
          mg_float = fmin(mg_float, fmin(mp_, mv_));
          pflip[a] = mp_ < FLIP_TAU ? (double)nextafterf(p, INFINITY) - (double)p : 0;
          vflip[a] = mv_ < FLIP_TAU ? (double)nextafterf(fabsf(v), INFINITY) - (double)fabsf(v) : 0;
          vsign[a] = vmag[a] > 0 && fabs(vd) < FLIP_TAU * vmag[a];
        }
      }
      double vel_norm =
          sqrt(vel[0] * vel[0] + vel[1] * vel[1] + vel[2] * vel[2]) + 1e-5;

      double dist, gd, cd, grad[3];
      double v8[8], vm8[8];
      if (boxes) {
        int low;
        dist = edt_query_ext(S, ext, pos, tau, grad, v8, vm8, &low);
        low_count += low;
      } else {
        dist = oracle_sdf_query(S, pos, grad);                     /* :363 */
      }
      cd = prm->alpha * exp(-(dist - prm->d0) / prm->r);           /* :509 */
      gd = -(prm->alpha / prm->r) * exp(-(dist - prm->d0) / prm->r); /* :514 */

      double Tm[6], TV[6], TVV[6];
      for (int i = 0; i < 6; ++i) Tm[i] = pow(t, i); /* :544-551 */
      /* T·V with V(i,i+1)=i+1, all else 0 (:104-105) */
      TV[0] = 0;
      for (int i = 1; i < 6; ++i) TV[i] = Tm[i - 1] * i;
      TVV[0] = 0;
      for (int i = 1; i < 6; ++i) TVV[i] = TV[i - 1] * i;

      cost_colli += cd * vel_norm * dt; /* :373 */

      double w1m[3] = {0, 0, 0}, w2m[3] = {0, 0, 0};
      if (mag) {
        double dm, gm[3], mgs[2], dgdp[3][3];
        sdf_query_mag_v(S, pos, boxes ? v8 : NULL, boxes ? vm8 : NULL, &dm, gm, mgs, dgdp);
        mg_cell = fmin(mg_cell, mgs[0]);
        mg_map = fmin(mg_map, mgs[1]);
        /* the exp argument's absolute error, in units of u: (|dist| + |d0|) / r */
        const double ec = 1 + (dm + fabs(prm->d0)) / fabs(prm->r);
        cm_c += fabs(cd) * ec * vel_norm * dt;
        for (int k = 0; k < 3; ++k) {
          /* mode 1: one exponential in the weight, not two */
          w1m[k] = cons ? fabs(gd * vel_norm) * (gm[k] + fabs(grad[k]) * ec)
                        : fabs(gd * cd * vel_norm) * (gm[k] + 2 * fabs(grad[k]) * ec);
          w2m[k] = fabs(cd) * ec * vmag[k] / vel_norm;   /* the velocity by its magnitude */
        }
        /* a coordinate whose float rounding can go either way (pre-rounding double within FLIP_TAU of its
         * magnitude from a rounding boundary): twice the first-order effect of one float step, absolute */
        double f1[3] = {0, 0, 0}, f2[3] = {0, 0, 0}, fc = 0;
        for (int j = 0; j < 3; ++j) {
          if (pflip[j] > 0) {
            const double dd = fabs(grad[j]) * pflip[j], rel = dd / fabs(prm->r);
            fc += fabs(cd) * rel * vel_norm;
            for (int k = 0; k < 3; ++k) {
              f1[k] += cons ? fabs(gd * vel_norm) * (fabs(grad[k]) * rel + dgdp[k][j] * pflip[j])
                            : fabs(gd * cd * vel_norm) * (2 * fabs(grad[k]) * rel + dgdp[k][j] * pflip[j]);
              f2[k] += fabs(cd) * rel * fabs(vel[k]) / vel_norm;
            }
          }
          if (vflip[j] > 0) {
            const double dvn = fabs(vel[j]) * vflip[j] / vel_norm;
            fc += fabs(cd) * dvn;
            for (int k = 0; k < 3; ++k) {
              f1[k] += (cons ? fabs(gd * grad[k]) : fabs(gd * grad[k] * cd)) * dvn;
              f2[k] += fabs(cd) * (fabs(vel[k]) * dvn / vel_norm + (k == j ? vflip[j] / vel_norm : 0));
            }
          }
        }
        if (fc > 0) {
          fl_c += 2 * fc * dt;
          for (int k = 0; k < 3; ++k)
            for (int cc = 0; cc < num_dp; ++cc) {
              double b = 0;
              for (int i = 0; i < 6; ++i) b += (f1[k] * Tm[i] + f2[k] * TV[i]) * fabs(Ldp[i * num_dp + cc]);
              fl_g[k * num_dp + cc] += 2 * b * dt;
            }
        }
      }

      for (int k = 0; k < 3; k++) { /* :376-381 */
        double s1 = cons ? gd * grad[k] * vel_norm : gd * grad[k] * cd * vel_norm;
        double s2 = cd * (vel[k] / vel_norm);
        for (int cc = 0; cc < num_dp; ++cc) {
          double a1 = 0, a2 = 0;
          for (int i = 0; i < 6; ++i) {
            a1 += (s1 * Tm[i]) * Ldp[i * num_dp + cc];
            a2 += (s2 * TV[i]) * Ldp[i * num_dp + cc];
          }
          g_colli[k * num_dp + cc] =
              g_colli[k * num_dp + cc] + (a1 + a2) * dt;
          if (mag) {
            double b = 0;
            for (int i = 0; i < 6; ++i)
              b += (w1m[k] * Tm[i] + w2m[k] * TV[i]) * fabs(Ldp[i * num_dp + cc]);
            gm_c[k * num_dp + cc] += b * dt;
          }
        }
      }

      /* dynamic-feasibility block, commented out in the reference
       * (:383-407); executed here only when enable_dyn != 0. */
      if (prm->enable_dyn && prm->step == 2) {
        double cv = 0, ca = 0, gv = 0, ga = 0, aflip[3] = {0, 0, 0};
        for (int a = 0; a < 3; ++a) { /* :491-505 */
          const double *q = c + 6 * a;
          double ad = 2 * q[2] + 6 * q[3] * pow(t, 1) + 12 * q[4] * pow(t, 2) +
                      20 * q[5] * pow(t, 3);
          float ac = ad;
          acc[a] = ac;
          if (mag) {
            const double ma_ = float_margin(ad, amag[a], 1);
            mg_float = fmin(mg_float, ma_);
            aflip[a] = ma_ < FLIP_TAU ? (double)nextafterf(fabsf(ac), INFINITY) - (double)fabsf(ac) : 0;
            asign[a] = amag[a] > 0 && fabs(ad) < FLIP_TAU * amag[a];
          }
        }
        double ev[3], ea[3];
        if (mag)
          for (int k = 0; k < 3; ++k) {
            ev[k] = 1 + (vmag[k] + fabs(prm->v0)) / fabs(prm->r_v);
            ea[k] = 1 + (amag[k] + fabs(prm->a0)) / fabs(prm->r_a);
          }
        /* the flip allowance through the exponentials: one float step of |v_k| / |a_k| moves the exponent by
         * step / r, one of any velocity moves vn */
        double fv[3] = {0, 0, 0}, fa[3] = {0, 0, 0}, dvr = 0;
        if (mag) {
          for (int k = 0; k < 3; ++k) {
            fv[k] = vflip[k] / fabs(prm->r_v);
            fa[k] = aflip[k] / fabs(prm->r_a);
            dvr += fabs(vel[k]) * vflip[k] / (vel_norm * vel_norm);
          }
        }
        double cvs[3], cas[3], Ssum = 0, Smag = 0, Sflip = 0; /* mode 1: every axis's penalty, their sum */
        for (int k = 0; k < 3; k++) {
          cv = prm->alpha_v * exp((fabs(vel[k]) - prm->v0) / prm->r_v); /* :519 */
          cost_vel += cv * vel_norm * dt;
          ca = prm->alpha_a * exp((fabs(acc[k]) - prm->a0) / prm->r_a); /* :529 */
          cost_acc += ca * vel_norm * dt;
          cvs[k] = cv;
          cas[k] = ca;
          if (mag) {
            Smag += fabs(cv) * ev[k] + fabs(ca) * ea[k];
            Sflip += fabs(cv) * fv[k] + fabs(ca) * fa[k];
            cm_v += fabs(cv) * ev[k] * vel_norm * dt;
            cm_a += fabs(ca) * ea[k] * vel_norm * dt;
            fl_cd += 2 * (fabs(cv) * (fv[k] + dvr) + fabs(ca) * (fa[k] + dvr)) * vel_norm * dt;
          }
        }
        for (int k = 0; k < 3; k++) {
          gv = (prm->alpha_v / prm->r_v) *
               exp((fabs(vel[k]) - prm->v0) / prm->r_v); /* :524 */
          ga = (prm->alpha_a / prm->r_a) *
               exp((fabs(acc[k]) - prm->a0) / prm->r_a); /* :534 */
          double s1 = gv * vel_norm, s2 = cv * (vel[k] / vel_norm);
          double s3 = ga * vel_norm, s4 = ca * (vel[k] / vel_norm);
          if (cons) { /* tests/consistent_twin.py: gv sgn(v_k) vn + S v_k / vn on T*V, ga sgn(a_k) vn on T*V*V */
            const double sv = (double)((vel[k] > 0) - (vel[k] < 0)), sa = (double)((acc[k] > 0) - (acc[k] < 0));
            Ssum = (cvs[0] + cvs[1] + cvs[2]) + (cas[0] + cas[1] + cas[2]);
            s1 = gv * sv * vel_norm;
            s2 = Ssum * (vel[k] / vel_norm);
            s3 = ga * sa * vel_norm;
            s4 = 0.0;
          }
          for (int cc = 0; cc < num_dp; ++cc) {
            double a1 = 0, a2 = 0, a3 = 0, a4 = 0;
            for (int i = 0; i < 6; ++i) {
              double l = Ldp[i * num_dp + cc];
              a1 += (s1 * TV[i]) * l;
              a2 += (s2 * TV[i]) * l;
              a3 += (s3 * TVV[i]) * l;
              a4 += (s4 * TV[i]) * l;
            }
            g_vel[k * num_dp + cc] += (a1 + a2) * dt;
            g_acc[k * num_dp + cc] += (a3 + a4) * dt;
            if (mag) {
              /* cv / ca: the last axis's values (the reference's loop variables) */
              double m1 = fabs(s1) * ev[k], m3 = fabs(s3) * ea[k];
              double m2 = fabs(cv) * ev[2] * vmag[k] / vel_norm, m4 = fabs(ca) * ea[2] * vmag[k] / vel_norm;
              if (cons) { /* S by the magnitudes of its six terms; an axis at exactly 0 (sgn = 0, vmag = 0) gets none */
                m2 = Smag * vmag[k] / vel_norm;
                m4 = 0.0;
              }
              double b1 = 0, b2 = 0;
              for (int i = 0; i < 6; ++i) {
                double l = fabs(Ldp[i * num_dp + cc]);
                b1 += (m1 + m2) * TV[i] * l;
                b2 += (m3 * TVV[i] + m4 * TV[i]) * l;
              }
              gm_v[k * num_dp + cc] += b1 * dt;
              gm_a[k * num_dp + cc] += b2 * dt;
              if (dvr > 0 || fv[k] > 0 || fa[k] > 0 || fv[2] > 0 || fa[2] > 0 || vflip[k] > 0 ||
                  (cons && (Sflip > 0 || vsign[k] || asign[k]))) {
                double e1 = fabs(s1) * (fv[k] + dvr), e3 = fabs(s3) * (fa[k] + dvr);
                double e2 = fabs(cv) * (fabs(vel[k]) * (fv[2] + 2 * dvr) + vflip[k]) / vel_norm;
                double e4 = fabs(ca) * (fabs(vel[k]) * (fa[2] + 2 * dvr) + vflip[k]) / vel_norm;
                if (cons) {
                  /* S moves with every axis's float step; the sign allowance: a velocity / acceleration whose
                   * pre-rounding double is within FLIP_TAU of its magnitude from zero may take another sgn in a correct
                   * implementation — its gv*vn / ga*vn term (doubled below with the rest) */
                  e2 = (fabs(Ssum) * (fabs(vel[k]) * 2 * dvr + vflip[k]) + fabs(vel[k]) * Sflip) / vel_norm;
                  e4 = 0.0;
                  if (vsign[k]) e1 += fabs(gv * vel_norm);
                  if (asign[k]) e3 += fabs(ga * vel_norm);
                }
                double b3 = 0;
                for (int i = 0; i < 6; ++i)
                  b3 += ((e1 + e2 + e4) * TV[i] + e3 * TVV[i]) * fabs(Ldp[i * num_dp + cc]);
                fl_gd[k * num_dp + cc] += 2 * b3 * dt;
              }
            }
          }
        }
      }
    }
    /* the `t < T` test: the last t inside and the first outside the bound */
    if (mag) {
      if (t_in > 0) mg_count = fmin(mg_count, fabs(T[s] - t_in) / T[s]);
      mg_count = fmin(mg_count, fabs(t - T[s]) / T[s]);
    }
    seg_start = seg_start + T[s];
  }
  if (nlowered) *nlowered = low_count;

  /* :412-418 */
  double ws = prm->ws, wc = prm->wc, wv = 1.0, wa = 1.0;
  if (prm->step == 1) ws = 0.0;
  double cost =
      ws * cost_smooth + wc * cost_colli + wv * cost_vel + wa * cost_acc + 1e-3;
  /* :425-432 */
  for (int a = 0; a < 3; ++a)
    for (int i = 0; i < num_dp; ++i)
      grad_out[i + num_dp * a] =
          (ws * g_smooth[a * num_dp + i] + wc * g_colli[a * num_dp + i] +
           wv * g_vel[a * num_dp + i] + wa * g_acc[a * num_dp + i]) +
          1e-5;
  if (mag) {
    const double wsm = fabs(ws), wcm = fabs(wc);
    mag[0] = wsm * cm_s + wcm * cm_c + cm_v + cm_a + 1e-3;
    for (int a = 0; a < 3; ++a)
      for (int i = 0; i < num_dp; ++i)
        mag[1 + i + num_dp * a] = wsm * gm_s[a * num_dp + i] + wcm * gm_c[a * num_dp + i] +
                                  gm_v[a * num_dp + i] + gm_a[a * num_dp + i] + 1e-5;
    double *mg = mag + 1 + 3 * num_dp;
    mg[0] = mg_float;
    mg[1] = mg_cell;
    mg[2] = mg_map;
    mg[3] = mg_count;
    double *fl = mg + 4;
    fl[0] = wcm * fl_c + fl_cd;
    for (int a = 0; a < 3; ++a)   /* (grad's layout: i + num_dp * a, as the accumulators') */
      for (int i = 0; i < num_dp; ++i) fl[1 + i + num_dp * a] = wcm * fl_g[a * num_dp + i] + fl_gd[a * num_dp + i];
    free(fl_g);
    free(fl_gd);
    free(cabs);
    free(gm_s);
    free(gm_c);
    free(gm_v);
    free(gm_a);
  }

  free(g_smooth);
  free(g_colli);
  free(g_vel);
  free(g_acc);
  free(d);
  free(coe);
  free(tmp);
  free(Ldp);
  return cost;
}

double oracle_cost_grad(int m, const double *L, const double *R,
                        const double *Df, const double *T,
                        const oracle_params *prm, const oracle_sdf *S,
                        const double *x, double *grad_out) {
  return cost_grad_impl(m, L, R, Df, T, prm, S, x, grad_out, NULL, NULL, 0.0, NULL);
}

double oracle_cost_grad_mag(int m, const double *L, const double *R,
                            const double *Df, const double *T,
                            const oracle_params *prm, const oracle_sdf *S,
                            const double *x, double *grad_out, double *mag) {
  return cost_grad_impl(m, L, R, Df, T, prm, S, x, grad_out, mag, NULL, 0.0, NULL);
}

double oracle_cost_grad_ext(int m, const double *L, const double *R, const double *Df, const double *T,
                            const oracle_params *prm, const oracle_sdf *S, const double *x, const oracle_ext *ext,
                            double t0, double *grad_out, double *mag) {
  return cost_grad_impl(m, L, R, Df, T, prm, S, x, grad_out, mag, ext, t0, NULL);
}

static double now_s(void) {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

/* Batch driver used by tests and by bench.py's cpu_baseline leg.
 * T: B×m (t_stride = m) or shared (t_stride = 0); Df: B×18; x, grad: B×n.
 * Setup (L, R per trajectory — what setPath does once per problem,
 * grad_traj_optimizer.cpp:88-98) is done first and NOT timed; `reps`
 * passes of the callback over all B trajectories are timed.
 * Returns seconds spent in the callbacks (all reps), or <0 on error. */
static double eval_batch_impl(int B, int m, const double *T, int t_stride,
                              const double *Df, const oracle_params *prm,
                              const oracle_sdf *S, const double *x, double *cost,
                              double *grad, double *mag, int reps, int nthreads, const oracle_ext *ext,
                              const double *t0, int t0_stride, int *lowered) {
  int nd = 3 * m + 3, n6 = 6 * m, n = 9 * (m - 1);
  size_t lsz = (size_t)n6 * nd, rsz = (size_t)nd * nd;
  int nprob = t_stride ? B : 1;
  double *Ls = dalloc(lsz * nprob), *Rs = dalloc(rsz * nprob);
  int err = 0;
  for (int b = 0; b < nprob; ++b)
    if (oracle_generator(m, T + (size_t)b * t_stride, NULL, NULL, NULL,
                         Ls + lsz * b, Rs + rsz * b) != 0)
      err = 1;
  if (err) {
    free(Ls);
    free(Rs);
    return -1.0;
  }
  if (nthreads < 1) nthreads = 1;
  double clk0 = now_s();
  for (int rep = 0; rep < reps; ++rep) {
#ifdef _OPENMP
#pragma omp parallel for num_threads(nthreads) schedule(static)
#endif
    for (int b = 0; b < B; ++b) {
      int p = t_stride ? b : 0;
      cost[b] = cost_grad_impl(m, Ls + lsz * p, Rs + rsz * p,
                               Df + (size_t)b * 18, T + (size_t)b * t_stride,
                               prm, S, x + (size_t)b * n, grad + (size_t)b * n,
                               mag ? mag + (size_t)b * (2 * n + 6) : NULL, ext,
                               t0 ? t0[(size_t)b * t0_stride] : 0.0, lowered ? lowered + b : NULL);
    }
  }
  double t1 = now_s();
  free(Ls);
  free(Rs);
  return t1 - clk0;
}

double oracle_eval_batch(int B, int m, const double *T, int t_stride,
                         const double *Df, const oracle_params *prm,
                         const oracle_sdf *S, const double *x, double *cost,
                         double *grad, int reps, int nthreads) {
  return eval_batch_impl(B, m, T, t_stride, Df, prm, S, x, cost, grad, NULL, reps, nthreads, NULL, NULL, 0, NULL);
}

double oracle_eval_batch_mag(int B, int m, const double *T, int t_stride,
                             const double *Df, const oracle_params *prm,
                             const oracle_sdf *S, const double *x, double *cost,
                             double *grad, double *mag, int nthreads) {
  return eval_batch_impl(B, m, T, t_stride, Df, prm, S, x, cost, grad, mag, 1, nthreads, NULL, NULL, 0, NULL);
}

double oracle_eval_batch_ext(int B, int m, const double *T, int t_stride, const double *Df, const oracle_params *prm,
                             const oracle_sdf *S, const double *x, const oracle_ext *ext, const double *t0,
                             int t0_stride, double *cost, double *grad, double *mag, int *lowered, int nthreads) {
  return eval_batch_impl(B, m, T, t_stride, Df, prm, S, x, cost, grad, mag, 1, nthreads, ext, t0, t0_stride, lowered);
}

/* ------------------------------------------------------------------ */
/* post-processing: PolynomialTraj                                     */
/* ------------------------------------------------------------------ */

/* include/grad_traj_optimization/polynomial_traj.hpp:46-66 — evaluate(t) on
 * coefficients in ASCENDING order c[0..5] (the node reverses them into
 * descending order, src/opti_node.cpp:118-120, and evaluate() pairs
 * tv(order-1-i) = pow(t,i) with them, i.e. a dot product that starts at t^5). */
static double traj_poly_eval(const double *c, double t) {
  double s = 0.0;
  for (int i = 5; i >= 0; --i) s += pow(t, (double)i) * c[i];
  return s;
}

/* out[9] = time_sum, length, jerk, mean_v, max_v, mean_a, max_a, acc_cost, n_samples.
 * coeff: m x 18 (row s = [cx0..5 | cy0..5 | cz0..5]).  dt_sample = 0.01 in the reference.
 * Convention where the reference has UB: evaluate() walks past the last segment when
 * t == time_sum exactly (:48-51); the last segment is extended instead. */
/* PolynomialTraj::getTraj, polynomial_traj.hpp:69-78: the points every dt_sample (0.01 in the reference), the
 * sample time accumulated; returns their number and stores the first max_samples of them. */
int oracle_traj_samples(int m, const double *coeff, const double *T, double dt_sample, int max_samples,
                        double *samples) {
  double time_sum = 0.0;
  for (int i = 0; i < m; ++i) time_sum += T[i];
  int nsamp = 0;
  for (double eval_t = 0.0; eval_t <= time_sum; eval_t += dt_sample) {
    double t = eval_t;
    int idx = 0;
    while (idx < m - 1 && T[idx] <= t) {
      t -= T[idx];
      ++idx;
    }
    if (nsamp < max_samples)
      for (int a = 0; a < 3; ++a) samples[3 * nsamp + a] = traj_poly_eval(coeff + idx * 18 + 6 * a, t);
    ++nsamp;
  }
  return nsamp;
}

void oracle_traj_stats(int m, const double *coeff, const double *T, double dt_sample, double *out) {
  double time_sum = 0.0; /* :37-43 */
  for (int i = 0; i < m; ++i) time_sum += T[i];

  double length = 0.0, pl[3] = {0, 0, 0}; /* getTraj :69-78 + getLength :80-92 */
  int nsamp = 0;
  for (double eval_t = 0.0; eval_t <= time_sum; eval_t += dt_sample) {
    double t = eval_t;
    int idx = 0;
    while (idx < m - 1 && T[idx] <= t) {
      t -= T[idx];
      ++idx;
    }
    double pn[3];
    for (int a = 0; a < 3; ++a) pn[a] = traj_poly_eval(coeff + idx * 18 + 6 * a, t);
    if (nsamp > 0) {
      double dx = pn[0] - pl[0], dy = pn[1] - pl[1], dz = pn[2] - pl[2];
      length += sqrt(dx * dx + dy * dy + dz * dz);
    }
    pl[0] = pn[0]; pl[1] = pn[1]; pl[2] = pn[2];
    ++nsamp;
  }

  double acc_cost = 0.0; /* getAccCost :96-109: um = 2*c[order-3] with descending c = 2*c2 */
  for (int s = 0; s < m; ++s) {
    double ux = 2 * coeff[s * 18 + 2], uy = 2 * coeff[s * 18 + 8], uz = 2 * coeff[s * 18 + 14];
    acc_cost += (ux * ux + uy * uy + uz * uz) * T[s];
  }

  double jerk = 0.0; /* getJerk :111-142 */
  for (int s = 0; s < m; ++s) {
    double M[6][6];
    memset(M, 0, sizeof(M));
    for (double i = 3; i < 6; i += 1)
      for (double j = 3; j < 6; j += 1)
        M[(int)i][(int)j] = i * (i - 1) * (i - 2) * j * (j - 1) * (j - 2) * pow(T[s], i + j - 5) / (i + j - 5);
    for (int a = 0; a < 3; ++a) {
      const double *c = coeff + s * 18 + 6 * a;
      double acc = 0.0; /* (c' M) c */
      for (int j = 3; j < 6; ++j) {
        double col = 0.0;
        for (int i = 3; i < 6; ++i) col += c[i] * M[i][j];
        acc += col * c[j];
      }
      jerk += acc;
    }
  }

  /* getMeanAndMaxVel :144-173, getMeanAndMaxAcc :175-204 — tv(i) = pow(ts, i): the
   * segment duration, not eval_t (kept as written) */
  double mean_v = 0.0, max_v = -1.0, mean_a = 0.0, max_a = -1.0;
  int num_v = 0, num_a = 0;
  for (int s = 0; s < m; ++s) {
    double vel[3], acc[3];
    for (int a = 0; a < 3; ++a) {
      const double *c = coeff + s * 18 + 6 * a;
      double sv = 0.0, sa = 0.0;
      for (int i = 0; i < 5; ++i) sv += pow(T[s], (double)i) * ((double)(i + 1) * c[i + 1]);
      for (int i = 0; i < 4; ++i) sa += pow(T[s], (double)i) * ((double)((i + 2) * (i + 1)) * c[i + 2]);
      vel[a] = sv;
      acc[a] = sa;
    }
    double vn = sqrt(vel[0] * vel[0] + vel[1] * vel[1] + vel[2] * vel[2]);
    double an = sqrt(acc[0] * acc[0] + acc[1] * acc[1] + acc[2] * acc[2]);
    for (double eval_t = 0.0; eval_t < T[s]; eval_t += dt_sample) {
      mean_v += vn;
      if (vn > max_v) max_v = vn;
      ++num_v;
      mean_a += an;
      if (an > max_a) max_a = an;
      ++num_a;
    }
  }
  mean_v = mean_v / (double)num_v;
  mean_a = mean_a / (double)num_a;

  out[0] = time_sum; out[1] = length; out[2] = jerk; out[3] = mean_v; out[4] = max_v;
  out[5] = mean_a; out[6] = max_a; out[7] = acc_cost; out[8] = (double)nsamp;
}

/* getCoefficientFromDerivative (src/grad_traj_optimizer.cpp:253-279): coe = L d, m x 18 */
void oracle_coefficients(int m, const double *L, const double *Df, const double *x, double *coe) {
  const int num_dp = 3 * m - 3, nd = 6 + num_dp, n6 = 6 * m;
  double *d = dalloc((size_t)nd);
  for (int a = 0; a < 3; ++a) {
    for (int j = 0; j < 6; ++j) d[j] = Df[a * 6 + j];
    for (int j = 0; j < num_dp; ++j) d[6 + j] = x[j + num_dp * a];
    for (int r = 0; r < n6; ++r) {
      double s = 0;
      for (int i = 0; i < nd; ++i) s += L[r * nd + i] * d[i];
      coe[(r / 6) * 18 + 6 * a + (r % 6)] = s;
    }
  }
  free(d);
}
