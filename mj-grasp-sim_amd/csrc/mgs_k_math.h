// mgs_k_math.h -- k_sincos, 3-vector / quaternion / spatial algebra, tree_sum, DofV.
#pragma once
#include "mgs_k_base.h"
// ---------------------------------------------------------------------------
// math primitives: identical expressions to the oracle
DEVI void k_sincos(double x, double* s, double* c) {
  const double inv_pio2 = 6.36619772367581382433e-01;
  const double pio2_1 = 1.57079632673412561417e+00;
  const double pio2_1t = 6.07710050650619224932e-11;
  const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03,
               S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
               S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
  const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03,
               C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
               C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
  double kd = x * inv_pio2;
  kd = (kd >= 0.0) ? floor(kd + 0.5) : -floor(0.5 - kd);
  double r = (x - kd * pio2_1) - kd * pio2_1t;
  double z = r * r;
  double ps = S1 + z * (S2 + z * (S3 + z * (S4 + z * (S5 + z * S6))));
  double sr = r + (r * z) * ps;
  double pc = C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6))));
  double cr = (1.0 - 0.5 * z) + (z * z) * pc;
  long k = (long)kd;
  int q = (int)(k & 3);
  if (q == 0) { *s = sr; *c = cr; }
  else if (q == 1) { *s = cr; *c = -sr; }
  else if (q == 2) { *s = -sr; *c = -cr; }
  else { *s = -cr; *c = sr; }
}

DEVI double dot3(const double* a, const double* b) {
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}
DEVI void cross3(double* r, const double* a, const double* b) {
  double r0 = a[1] * b[2] - a[2] * b[1];
  double r1 = a[2] * b[0] - a[0] * b[2];
  double r2 = a[0] * b[1] - a[1] * b[0];
  r[0] = r0; r[1] = r1; r[2] = r2;
}
DEVI void sub3(double* r, const double* a, const double* b) {
  r[0] = a[0] - b[0]; r[1] = a[1] - b[1]; r[2] = a[2] - b[2];
}
DEVI void add3(double* r, const double* a, const double* b) {
  r[0] = a[0] + b[0]; r[1] = a[1] + b[1]; r[2] = a[2] + b[2];
}
DEVI void mulmv3(double* r, const double* m, const double* v) {
  double r0 = (m[0] * v[0] + m[1] * v[1]) + m[2] * v[2];
  double r1 = (m[3] * v[0] + m[4] * v[1]) + m[5] * v[2];
  double r2 = (m[6] * v[0] + m[7] * v[1]) + m[8] * v[2];
  r[0] = r0; r[1] = r1; r[2] = r2;
}
DEVI void mulmtv3(double* r, const double* m, const double* v) {
  double r0 = (m[0] * v[0] + m[3] * v[1]) + m[6] * v[2];
  double r1 = (m[1] * v[0] + m[4] * v[1]) + m[7] * v[2];
  double r2 = (m[2] * v[0] + m[5] * v[1]) + m[8] * v[2];
  r[0] = r0; r[1] = r1; r[2] = r2;
}
DEVI void quatmul(double* r, const double* a, const double* b) {
  double r0 = ((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3];
  double r1 = ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2];
  double r2 = ((a[0] * b[2] - a[1] * b[3]) + a[2] * b[0]) + a[3] * b[1];
  double r3 = ((a[0] * b[3] + a[1] * b[2]) - a[2] * b[1]) + a[3] * b[0];
  r[0] = r0; r[1] = r1; r[2] = r2; r[3] = r3;
}
DEVI void quat2mat(double* m, const double* q) {
  double q00 = q[0] * q[0], q01 = q[0] * q[1], q02 = q[0] * q[2], q03 = q[0] * q[3];
  double q11 = q[1] * q[1], q12 = q[1] * q[2], q13 = q[1] * q[3];
  double q22 = q[2] * q[2], q23 = q[2] * q[3], q33 = q[3] * q[3];
  m[0] = ((q00 + q11) - q22) - q33;
  m[1] = 2.0 * (q12 - q03);
  m[2] = 2.0 * (q13 + q02);
  m[3] = 2.0 * (q12 + q03);
  m[4] = ((q00 - q11) + q22) - q33;
  m[5] = 2.0 * (q23 - q01);
  m[6] = 2.0 * (q13 - q02);
  m[7] = 2.0 * (q23 + q01);
  m[8] = ((q00 - q11) - q22) + q33;
}
DEVI void normalize4(double* q) {
  double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  if (n < K_MINVAL) { q[0] = 1.0; q[1] = q[2] = q[3] = 0.0; return; }
  double inv = 1.0 / n;
  q[0] = q[0] * inv; q[1] = q[1] * inv; q[2] = q[2] * inv; q[3] = q[3] * inv;
}
DEVI double normalize3(double* v) {
  double n = sqrt(dot3(v, v));
  if (n < K_MINVAL) { v[0] = 1.0; v[1] = v[2] = 0.0; return 0.0; }
  double inv = 1.0 / n;
  v[0] = v[0] * inv; v[1] = v[1] * inv; v[2] = v[2] * inv;
  return n;
}
DEVI void axisangle2quat(double* q, const double* axis, double angle) {
  double s, c;
  k_sincos(0.5 * angle, &s, &c);
  q[0] = c; q[1] = axis[0] * s; q[2] = axis[1] * s; q[3] = axis[2] * s;
}
DEVI void mul_inert_vec(double* r, const double* i, const double* v) {
  double r0 = ((i[0] * v[0] + i[3] * v[1]) + i[4] * v[2]) - i[8] * v[4] + i[7] * v[5];
  double r1 = ((i[3] * v[0] + i[1] * v[1]) + i[5] * v[2]) + i[8] * v[3] - i[6] * v[5];
  double r2 = ((i[4] * v[0] + i[5] * v[1]) + i[2] * v[2]) - i[7] * v[3] + i[6] * v[4];
  double r3 = (i[8] * v[1] - i[7] * v[2]) + i[9] * v[3];
  double r4 = (i[6] * v[2] - i[8] * v[0]) + i[9] * v[4];
  double r5 = (i[7] * v[0] - i[6] * v[1]) + i[9] * v[5];
  r[0] = r0; r[1] = r1; r[2] = r2; r[3] = r3; r[4] = r4; r[5] = r5;
}
DEVI double dot6(const double* a, const double* b) {
  return ((((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]) + a[4] * b[4]) + a[5] * b[5];
}
DEVI void cross_motion(double* r, const double* v, const double* u) {
  double r0 = v[1] * u[2] - v[2] * u[1];
  double r1 = v[2] * u[0] - v[0] * u[2];
  double r2 = v[0] * u[1] - v[1] * u[0];
  double r3 = (v[1] * u[5] - v[2] * u[4]) + (v[4] * u[2] - v[5] * u[1]);
  double r4 = (v[2] * u[3] - v[0] * u[5]) + (v[5] * u[0] - v[3] * u[2]);
  double r5 = (v[0] * u[4] - v[1] * u[3]) + (v[3] * u[1] - v[4] * u[0]);
  r[0] = r0; r[1] = r1; r[2] = r2; r[3] = r3; r[4] = r4; r[5] = r5;
}
DEVI void cross_force(double* r, const double* v, const double* f) {
  double r0 = (v[1] * f[2] - v[2] * f[1]) + (v[4] * f[5] - v[5] * f[4]);
  double r1 = (v[2] * f[0] - v[0] * f[2]) + (v[5] * f[3] - v[3] * f[5]);
  double r2 = (v[0] * f[1] - v[1] * f[0]) + (v[3] * f[4] - v[4] * f[3]);
  double r3 = v[1] * f[5] - v[2] * f[4];
  double r4 = v[2] * f[3] - v[0] * f[5];
  double r5 = v[0] * f[4] - v[1] * f[3];
  r[0] = r0; r[1] = r1; r[2] = r2; r[3] = r3; r[4] = r4; r[5] = r5;
}

// Pairwise tree reduction over lanes, identical to the oracle's tree_dot():
// level s (s = 1, 2, 4, ... < P) adds lane k^s to lane k.  Within a 16-lane row
// the levels are DPP moves (xor 1 and xor 2 by quad permutes; xor 4 and xor 8 by
// the half-row / row mirrors, which equal xor on values already uniform over
// the lower levels); the last two levels combine the four row sums read with
// v_readlane in the same pairing ((r0 + r1) + (r2 + r3)).  Result is uniform.
DEVI double dpp_d(double x, int ctrl_sel) {
  int lo = __double2loint(x), hi = __double2hiint(x);
  switch (ctrl_sel) {
    case 0: lo = __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, false); hi = __builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, false); break;
    case 1: lo = __builtin_amdgcn_mov_dpp(lo, 0x4E, 0xF, 0xF, false); hi = __builtin_amdgcn_mov_dpp(hi, 0x4E, 0xF, 0xF, false); break;
    case 2: lo = __builtin_amdgcn_mov_dpp(lo, 0x141, 0xF, 0xF, false); hi = __builtin_amdgcn_mov_dpp(hi, 0x141, 0xF, 0xF, false); break;
    default: lo = __builtin_amdgcn_mov_dpp(lo, 0x140, 0xF, 0xF, false); hi = __builtin_amdgcn_mov_dpp(hi, 0x140, 0xF, 0xF, false); break;
  }
  return __hiloint2double(hi, lo);
}
DEVI double readlane_d(double x, int l) {
  int lo = __builtin_amdgcn_readlane(__double2loint(x), l);
  int hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
  return __hiloint2double(hi, lo);
}
DEVI double tree_sum(double leaf, int P) {
  if (P > 1) leaf = leaf + dpp_d(leaf, 0);
  if (P > 2) leaf = leaf + dpp_d(leaf, 1);
  if (P > 4) leaf = leaf + dpp_d(leaf, 2);
  if (P > 8) leaf = leaf + dpp_d(leaf, 3);
  if (P > 16) {
    double r0 = readlane_d(leaf, 0), r1 = readlane_d(leaf, 16);
    if (P > 32) {
      double r2 = readlane_d(leaf, 32), r3 = readlane_d(leaf, 48);
      return (r0 + r1) + (r2 + r3);
    }
    return r0 + r1;
  }
  return readlane_d(leaf, 0);
}
DEVI int next_pow2(int n) {
  int P = 1;
  while (P < n) P <<= 1;
  return P;
}

// Dofs per lane.  Lanes over dofs is the unit of the dynamics, the solves and
// the solver sweeps: lane l owns dof l (MGS_DPL 1, every library build and
// every model of at most 64 dofs) or dofs l and l + 64 (MGS_DPL 2: the
// specialised objects of models with 65-128 dofs, clutter piles of 7-10
// objects).  A dof-indexed value held in registers is a DofV; with MGS_DPL 1
// every helper below is the single-slot expression it replaces.
#ifndef MGS_DPL
#define MGS_DPL 1
#endif
static_assert(MGS_DPL == 1 || MGS_DPL == 2, "MGS_DPL is 1 or 2");
static_assert(MGS_DPL == 1 || (MGS_PACKED && !MGS_REG_ROWS), "two dofs per lane: the wide flavour (MGS_WIDE)");
#define MGS_MAXNV (WAVE * MGS_DPL)
struct DofV {
  double v[MGS_DPL];
};
DEVI DofV dof_zero() {
  DofV x;
#pragma unroll
  for (int h = 0; h < MGS_DPL; h++) x.v[h] = 0.0;
  return x;
}
// p[dof] on the dof's lane, 0 past nv
DEVI DofV dof_load(const double* p, int nv, int lane) {
  DofV x;
#pragma unroll
  for (int h = 0; h < MGS_DPL; h++) x.v[h] = (lane + h * WAVE < nv) ? p[lane + h * WAVE] : 0.0;
  return x;
}
DEVI DofV dof_mul(const DofV& a, const DofV& b) {
  DofV x;
#pragma unroll
  for (int h = 0; h < MGS_DPL; h++) x.v[h] = a.v[h] * b.v[h];
  return x;
}
// the oracle's tree_dot over the dof leaves (P = next_pow2(nv)): a tree over
// 128 leaves is the tree over dofs 0-63 plus the tree over dofs 64-127 (its
// last level adds leaf 64 to leaf 0)
DEVI double dof_tree(const DofV& x, int P) {
  if (MGS_DPL == 1 || P <= WAVE) return tree_sum(x.v[0], P);
  return tree_sum(x.v[0], WAVE) + tree_sum(x.v[MGS_DPL - 1], WAVE);
}
// u += g delta on the lanes' dofs below nv (the others keep their value)
DEVI void dof_axpy(DofV& u, const DofV& g, double delta, int nv, int lane) {
#pragma unroll
  for (int h = 0; h < MGS_DPL; h++) {
    double s = u.v[h] + g.v[h] * delta;
    if (lane + h * WAVE < nv) u.v[h] = s;
  }
}
// `DOF_SLOTS(i, nv) stmt;`: stmt for each dof i < nv of this lane (lane, lane + 64)
#define DOF_SLOTS(i, nv) \
  _Pragma("unroll") for (int _h = 0, i = lane + 0; _h < MGS_DPL; _h++, i += WAVE) if (i < (nv))
// dof k's value, uniform (k uniform)
DEVI double dof_readlane(const DofV& x, int k) {
  if (MGS_DPL == 1) return readlane_d(x.v[0], k);
  return readlane_d((k >> 6) ? x.v[MGS_DPL - 1] : x.v[0], k & (WAVE - 1));
}
// dof col moves body b: the model's body_dofmask, bit col of the body's words
// (2 words per body, 4 for models of more than 64 dofs; mgs_gpu.h)
DEVI int dof_moves(const Mdl& md, int b, int col) {
  if (MGS_DPL == 1) {
    const int32_t* mask = IA(md, body_dofmask) + 2 * b;
    return (col < 32) ? ((mask[0] >> col) & 1) : ((mask[1] >> (col - 32)) & 1);
  }
  const int32_t* mask = IA(md, body_dofmask) + (md.m.nv > 64 ? 4 : 2) * b;
  return (mask[col >> 5] >> (col & 31)) & 1;
}

