// mgs_k_base.h -- the C-ABI header, K_* constants, the model and LDS views (Mdl,
// Dat), the build switches (MGS_RPL, MGS_GPAD, MGS_MAXDIM, MGS_REG_ROWS,
// MGS_PACKED, MGS_MU_MODEL), DEVI, lane_id / uni / shfl, the stage timers, wsync.
#pragma once
// the wide flavour (-DMGS_WIDE, clutter piles): 4 constraint rows per lane, G rows in HBM
#ifdef MGS_WIDE
#define MGS_RPL 4
#ifndef MGS_G_LDS          /* -DMGS_G_LDS: the wide build with G kept in LDS (experiments) */
#define MGS_G_GLOBAL 1
#endif
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mgs_gpu.h"

#define K_MINVAL 1e-15
#define K_MAXF 16
#define K_MAXPOLY 40
#define K_POLY_POINTS (4 * K_MAXF + 3 * K_MAXPOLY)   // collide_manifold's polygon scratch
#define K_MPR_MAXIT 64
#define K_FEAT_EPS 1e-5
#define K_BB_MERGE 1e-6     // box-box: merge distance of manifold points, x face half size (oracle BB_MERGE)
// separation certificates (cert_check): slots per candidate, doubles per slot,
// the least margin worth keeping and the safety margin of the validity test
#define K_CERT 8
#define CERT_W 17
#define CERT_STORE 1e-6
#define CERT_EPS 1e-10
#define WAVE 64
// row stride of the constraint matrix G (doubles): NV + MGS_GPAD.  With lanes
// over rows reading G[r * GS + k], an odd stride spreads the 32 lanes of a
// ds_read_b64 group over distinct banks (pad 1, the default with G in LDS, at
// the even dof counts of the shipped models).  G rows in HBM are unpadded
#ifndef MGS_GPAD
#ifdef MGS_G_GLOBAL
#define MGS_GPAD 0
#else
#define MGS_GPAD 1
#endif
#endif
#define GS (NV + MGS_GPAD)
#if defined(MGS_G_GLOBAL) && MGS_GPAD != 0
#error "G rows in HBM are unpadded (launch_layout sizes them nefc_max * nv)"
#endif
#define DEVI __device__ __attribute__((always_inline)) inline

struct P2 { double x, y, h; };

// ---------------------------------------------------------------------------
// model access
struct Mdl {
  mgs_model_desc m;
  const int32_t* I;
  const double* D;
};
#define IA(md, f) ((md).I + (md).m.i_##f)
#define DA(md, f) ((md).D + (md).m.d_##f)

// per-candidate working set in LDS (see make_layout in mgs_capi.hip for the
// carve-up; the U region is time-multiplexed between pipeline stages)
struct Dat {
  double *qpos, *qvel, *qacc_ws, *ctrl, *mocap_pos, *mocap_quat, *time;
  double *act, *act_dot;   // actuator state (mujoco.pid setpoint / integral) and its rate (ABI 21)
  double *xpos, *xquat, *xmat, *xipos, *xanchor, *xaxis;
  double *subtree_com, *subtree_mass, *cinert, *cdof;
  double *geom_xpos, *geom_xmat;
  double *M, *Dv, *Dinv, *sD, *isD, *tmp, *tmp2;
  double *qfrc_bias, *qfrc_passive, *qfrc_actuator, *qfrc_smooth, *qacc_smooth, *qfrc_constraint;
  double *act_force, *act_moment, *act_length, *act_vel;
  double *con_pos, *con_frame, *con_dist;
  double *efc_R, *efc_b, *con_mu, *con_blk;
  double* cert;     // separation certificates (K_CERT slots of CERT_W doubles, see cert_check)
  // U region views
  double *crb, *cvel, *cacc, *cfrc, *cdof_dot;          // dynamics stage
  P2* poly;                                           // collision stage
  double* pdep;                                       // collision stage
  double *comacc;                                     // comPos stage
  double *G, *efc_aref, *efc_vel, *efc_pos, *efc_margin, *scratch;  // constraint + solver stage
  double* qDeriv;                                     // integration stage
  // Newton solver workspace (U region, after the constraint stage views)
  double *efc_jar, *efc_jv, *efc_f, *efc_Dr, *efc_isR, *nH, *nw, *nw0, *ng, *ndir, *con_hb;
  int *con_pair, *con_g1, *con_g2, *efc_type, *efc_dim, *efc_con, *efc_state, *ints;
  int gs;   // row stride of G (nv + 1)
};
// ints[]: 0 ncon, 1 nefc, 2 overflow, 3 iters, 6 cr0, 7 cr1, 8 neq rows, 9 fr0, 10 fr1, 11 lr0, 12 lr1
#define NCON ints[0]
#define NEFC ints[1]
#define OVERFLOW ints[2]
#define ITERS ints[3]
// largest contact dimension the kernels handle: 4 (frictionless, sliding,
// torsional) in the libraries and most specialised objects; 6 (rolling too)
// in the objects of models with condim-6 pairs (mgs/core/special.py,
// -DMGS_MAXDIM=6).  Per-contact block storage is MGS_MAXDIM^2 doubles.
#ifndef MGS_MAXDIM
#define MGS_MAXDIM 4
#endif
static_assert(MGS_MAXDIM == 4 || MGS_MAXDIM == 6, "MGS_MAXDIM is 4 or 6");
#define BLKSTRIDE (MGS_MAXDIM * MGS_MAXDIM)
#ifndef MGS_RPL
#define MGS_RPL 2   // constraint rows per lane (nefc_max <= 64 * MGS_RPL)
#endif
// NV-long operand rows of the factor, the triangular solves and the G
// products held in registers, or read from LDS at each use.  Registers in
// every build of one dof per lane: the wide flavour's pile objects (nv 38-58,
// one wave per SIMD) hold them in 424 VGPRs without spilling, and the C5 pile
// rollout runs 6 % faster for it (round 5, profiles/r05w_c5_register_rows_ab.txt);
// with two dofs per lane (MGS_DPL 2) each lane has two rows: LDS.  Same values
// either way.
#ifndef MGS_REG_ROWS
#if defined(MGS_DPL) && MGS_DPL > 1
#define MGS_REG_ROWS 0
#else
#define MGS_REG_ROWS 1
#endif
#endif

// Packed storage of the mass matrix / its LDL factor and of the Newton
// Hessian (symmetric; only the lower triangle is ever read): row i of the
// lower triangle at i (i + 1) / 2 instead of i nv.  The wide build (clutter
// piles, nv up to 58, whose row loops read M and H from LDS anyway) packs
// them: 2 x 1653 doubles less at nv 58 (round 5, two pile workgroups per CU);
// the main build keeps the square layout its register-row factor loads.
#ifndef MGS_PACKED
#ifdef MGS_WIDE
#define MGS_PACKED 1
#else
#define MGS_PACKED 0
#endif
#endif
#if MGS_PACKED
#define TRI(i, k, n) ((((i) * ((i) + 1)) >> 1) + (k))
#define TRI_SIZE(n) (((n) * ((n) + 1)) >> 1)
#else
#define TRI(i, k, n) ((i) * (n) + (k))
#define TRI_SIZE(n) ((n) * (n))
#endif
// (the register-row factor and solves load row i's lower entries by TRI too;
// the upper ones they load are never used, and TRI keeps them in bounds)
// the friction coefficients of a contact: its pair's row of the model instead
// of a per-contact copy in LDS (main-library objects with G in HBM, round 5:
// the same values -- the copy's one extra slot, mu[dim - 1] = 0, is never read)
#ifndef MGS_MU_MODEL
#define MGS_MU_MODEL 0
#endif

// the lane index through an opaque move at every use: index arithmetic and
// lane masks derived from it are recomputed where they are used instead of
// being hoisted out of the step loop and held (in VGPRs, AGPRs and SGPR
// spill lanes) for the whole rollout (round 5: the headline rollout 430 ->
// 328 registers with this alone; profiles/r05c_ab.txt)
DEVI int lane_id() {
  int l = (int)__lane_id();
  asm volatile("" : "+v"(l));
  return l;
}
// values that are uniform across the wave but come from LDS: move to SGPRs so
// control flow on them is scalar
DEVI int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }

// wave-wide shuffle from lane src (0..63): HIP's __shfl(x, src) with width 64
// (ds_bpermute at byte address 4 src), without its lane-index term, so no
// per-lane address is derived from the lane index and held across the step loop
DEVI int shfl(int x, int src) { return __builtin_amdgcn_ds_bpermute(src << 2, x); }
DEVI double shfl(double x, int src) {
  const int a = src << 2;
  const int lo = __builtin_amdgcn_ds_bpermute(a, __double2loint(x));
  const int hi = __builtin_amdgcn_ds_bpermute(a, __double2hiint(x));
  return __hiloint2double(hi, lo);
}

// Diagnostic stage timers (built only with -DMGS_PROFILE; never in the product build)
#ifdef MGS_PROFILE
#ifdef MGS_SPECIAL
// a specialised code object's timers, read by the host with hipModuleGetGlobal
extern "C" {
__device__ unsigned long long g_prof[64];
}
#else
// one copy per translation unit (each dof count's kernels, mgs_inst.hip)
static __device__ unsigned long long g_prof[64];
#endif
// per-workgroup accumulators in static LDS; PT(k) at wave-uniform points only
__shared__ unsigned long long s_prof[67];
#define PT(k) do { unsigned long long _n = __builtin_amdgcn_s_memtime(); \
    if (__lane_id() == 0) { s_prof[k] += _n - s_prof[64]; s_prof[64] = _n; } } while (0)
// slots 61 / 62 at the flush: the workgroup's shader-clock and 100 MHz
// real-time spans (their ratio is the clock the chip held, MI355X_MICROARCH.md
// "DVFS give-back" item 6)
#define PROF_DECL if (__lane_id() == 0) { for (int _k = 0; _k < 64; _k++) s_prof[_k] = 0; \
    s_prof[64] = s_prof[65] = __builtin_amdgcn_s_memtime(); s_prof[66] = __builtin_amdgcn_s_memrealtime(); }
#define PROF(k) PT(k)
#define PCNT(k, v) do { if (__lane_id() == 0) s_prof[k] += (v); } while (0)
#define PROF_FLUSH if (lane_id() == 0) { \
    s_prof[61] = __builtin_amdgcn_s_memtime() - s_prof[65]; \
    s_prof[62] = __builtin_amdgcn_s_memrealtime() - s_prof[66]; \
    for (int _k = 0; _k < 64; _k++) atomicAdd(&g_prof[_k], s_prof[_k]); }
#else
#define PT(k)
#define PROF_DECL
#define PROF(k)
#define PCNT(k, v)
#define PROF_FLUSH
#endif
// Lane-to-lane hand-off inside the one-wave workgroup.  Main build: every
// such hand-off goes through LDS, whose operations a wave issues and the LDS
// processes in order, so a wavefront-scope fence (it keeps the compiler from
// moving memory operations across it) is enough: +1 % on the bench, -1 % on
// one API launch (profiles/r04v_wavefront_fence_ab.txt).  Wide build (G in
// HBM: rows written by lanes over rows and read by lanes over dofs through
// global memory): the workgroup barrier, which waits for the stores.
#if defined(MGS_WSYNC_FENCE) || (!defined(MGS_G_GLOBAL) && !defined(MGS_WSYNC_BARRIER))
DEVI void wsync() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }
#else
DEVI void wsync() { __syncthreads(); }
#endif

