// mgs_capi.hip -- host side of libmgs_gpu.so: the C-ABI declared in
// include/mgs_gpu.h (model upload, batch buffers, kernel launches, timing).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "mgs_kernels.hip"
#include "mgs_launch.h"
#include "mgs_aux.hip"
#include "mgs_sampler.hip"
#include "mgs_scan.hip"
#include "mgs_contact.hip"
#include "mgs_cloud.hip"
#include "mgs_pose.hip"

#include <cstdlib>

#define MGS_QUEUE_RING 64

namespace {
thread_local std::string g_err;

int fail(int code, const char* fmt, const char* what = "") {
  char buf[512];
  snprintf(buf, sizeof(buf), fmt, what);
  g_err = buf;
  return code;
}

#define HIPCHK(expr)                                                                  \
  do {                                                                                \
    hipError_t _e = (expr);                                                           \
    if (_e != hipSuccess) return fail(MGS_EHIP, "HIP error: %s", hipGetErrorString(_e)); \
  } while (0)

// written so that a NaN fails
bool is_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// The host layer's rule: the device memory of one call lives in a DevBufs,
// freed on every return path; mgs_model and mgs_batch own theirs
// (mgs_model_free, mgs_batch_close); launches name their arguments.
struct DevBufs {
  std::vector<void*> p;
  bool ok = true;
  template <class T>
  T* get(size_t n) {
    void* q = nullptr;
    if (hipMalloc(&q, (n > 0 ? n : 1) * sizeof(T)) != hipSuccess) { ok = false; return nullptr; }
    p.push_back(q);
    return (T*)q;
  }
  ~DevBufs() { for (void* q : p) hipFree(q); }
};
// a host array on the device (b.ok turns false when the allocation or the copy fails)
template <class T>
T* upload(DevBufs& b, const T* src, size_t n) {
  T* d = b.get<T>(n);
  if (d && n > 0 && hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) b.ok = false;
  return d;
}
// the time between its construction and finish() on the null stream
struct EvTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  EvTimer() { hipEventCreate(&e0); hipEventCreate(&e1); hipEventRecord(e0, nullptr); }
  int finish(double* ms) {
    hipEventRecord(e1, nullptr);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e != hipSuccess) return fail(MGS_EHIP, "HIP error: %s", hipGetErrorString(e));
    float f = 0.f;
    hipEventElapsedTime(&f, e0, e1);
    if (ms) *ms = f;
    return MGS_OK;
  }
  ~EvTimer() { hipEventDestroy(e0); hipEventDestroy(e1); }
};

// whether a model's G rows live in HBM
#ifdef MGS_G_GLOBAL
bool g_in_hbm(const mgs_model_desc&) { return true; }
#else
bool g_in_hbm(const mgs_model_desc& m) { return m.g_rows_hbm != 0; }
#endif

// main-library objects with G in HBM also pack M / the Newton Hessian and read
// the contacts' friction from the model (-DMGS_PACKED=1 -DMGS_MU_MODEL=1,
// mgs/core/special.py), so that six headline candidates fit a CU
int m_square_size(const mgs_model_desc& m) {
  const int nv = m.nv;
  return (MGS_PACKED || m.g_rows_hbm) ? nv * (nv + 1) / 2 : nv * nv;
}
bool mu_from_model(const mgs_model_desc& m) { return !MGS_PACKED && m.g_rows_hbm; }
// ... and keep certificates, contact frames and contact blocks in the HBM
// slice (-DMGS_HBM_EXTRA=1): seven headline candidates per CU
bool hbm_extra(const mgs_model_desc& m) { return !MGS_PACKED && m.g_rows_hbm; }
int layout_maxdim(const mgs_model_desc& m);
size_t hbm_slice_doubles(const mgs_model_desc& m) {
  const int md = layout_maxdim(m);
  // (... and the copy of M that integrate restores: the kernel's hbm_slice)
  return (size_t)m.nefc_max * m.nv +
         (hbm_extra(m) ? (size_t)(K_CERT * CERT_W + 9 * m.ncon_max + md * md * m.ncon_max + m_square_size(m)) : 0);
}

// the contact dimension the kernels for this model are built for (MGS_MAXDIM)
int layout_maxdim(const mgs_model_desc& m) { return m.maxcondim > 4 ? 6 : 4; }

// LDS carve-up of one candidate's working set (doubles, then int counters and
// index arrays).  U is time-multiplexed: collision scratch, then composite
// inertias / RNE temporaries, then constraint rows (G) + solver scratch, then
// the integrator's derivative matrix.
Lay make_layout(const mgs_model_desc& m, size_t* bytes) {
  Lay l;
  memset(&l, 0, sizeof(l));
  int nq = m.nq, nv = m.nv, nb = m.nbody, ng = m.ngeom, nu = m.nu > 0 ? m.nu : 1;
  int nj = m.njnt > 0 ? m.njnt : 1, nc = m.ncon_max, ne = m.nefc_max;
  int sizes[L_COUNT];
  sizes[L_qpos] = nq; sizes[L_qvel] = nv; sizes[L_qacc_ws] = nv; sizes[L_ctrl] = nu;
  sizes[L_mocap_pos] = 3 * m.nmocap + 3; sizes[L_mocap_quat] = 4 * m.nmocap + 4; sizes[L_time] = 1;
  sizes[L_act] = m.nact; sizes[L_act_dot] = m.nact;
  sizes[L_xpos] = 3 * nb; sizes[L_xquat] = 4 * nb; sizes[L_xmat] = 9 * nb; sizes[L_subtree_com] = 3 * nb;
  sizes[L_cinert] = 10 * nb; sizes[L_cdof] = 6 * nv;
  sizes[L_M] = m_square_size(m); sizes[L_Dv] = nv; sizes[L_Dinv] = nv; sizes[L_sD] = nv; sizes[L_isD] = nv;
  sizes[L_tmp] = nv; sizes[L_tmp2] = nv;
  sizes[L_qfrc_smooth] = nv; sizes[L_qacc_smooth] = nv; sizes[L_qfrc_constraint] = nv;
  // (the wide build reads the actuator moment rows from the model)
  sizes[L_act_force] = nu; sizes[L_act_moment] = MGS_PACKED ? 0 : nu * nv; sizes[L_act_length] = nu; sizes[L_act_vel] = nu;
  sizes[L_con_pos] = 3 * nc; sizes[L_con_frame] = hbm_extra(m) ? 0 : 9 * nc; sizes[L_con_dist] = nc; sizes[L_con_mu] = mu_from_model(m) ? 0 : 5 * nc;
  // contact blocks (and Newton cone Hessians): maxdim^2 per contact, maxdim 6
  // for models with condim-6 pairs (their code objects: -DMGS_MAXDIM=6)
  const int maxdim = layout_maxdim(m);
  sizes[L_con_blk] = hbm_extra(m) ? 0 : maxdim * maxdim * nc;
  sizes[L_efc_R] = ne; sizes[L_efc_b] = ne; sizes[L_cert] = hbm_extra(m) ? 0 : K_CERT * CERT_W;
  // U: per-stage sub-layouts, each packed from offset 0 (see the kernel's Lay comment)
  int us[U_COUNT];
  for (int k = 0; k < U_COUNT; k++) us[k] = 0;
  us[U_poly] = K_POLY_POINTS * 3; us[U_pdep] = K_MAXPOLY; us[U_geom_xpos] = 3 * ng; us[U_geom_xmat] = 9 * ng;
  us[U_xipos] = 3 * nb; us[U_xanchor] = 3 * nj; us[U_xaxis] = 3 * nj; us[U_subtree_mass] = nb;
  us[U_comacc] = 4 * nb;
  us[U_cvel] = 6 * nb; us[U_cacc] = 6 * nb; us[U_cfrc] = 6 * nb; us[U_cdof_dot] = 6 * nv;
  us[U_qfrc_bias] = nv; us[U_qfrc_passive] = nv; us[U_qfrc_actuator] = nv;
  // G in HBM (batch buffer, see bind()): the wide library always, the main
  // library's specialised objects on request (mgs_model_desc.g_rows_hbm)
  us[U_G] = g_in_hbm(m) ? 0 : ne * (nv + MGS_GPAD);   // row stride: GS in the kernel
  us[U_aref] = ne;
  us[U_scratch] = (2 * ne > nv ? 2 * ne : nv);
  // {vel, pos, margin} (make_constraints) | Newton Hessian, which may run on into
  // the scratch slot (scratch is idle while the Hessian is live)
  // (the Hessian's weight table, (maxdim + 1) ne, runs on into scratch too)
  int xreg = 3 * ne;
  if (xreg + us[U_scratch] < (maxdim + 1) * ne) xreg = (maxdim + 1) * ne - us[U_scratch];
  if (xreg + us[U_scratch] < m_square_size(m)) xreg = m_square_size(m) - us[U_scratch];
  us[U_jar] = ne; us[U_jv] = ne; us[U_f] = ne; us[U_Dr] = ne; us[U_isR] = ne;
  us[U_nw] = nv; us[U_nw0] = nv; us[U_ng] = nv; us[U_ndir] = nv;
  int U = 0, off;
  // kin / collision stage
  off = 0;
  for (int k = U_poly; k <= U_comacc; k++) { l.u[k] = off; off += us[k]; }
  if (off > U) U = off;
  // dynamics: crb alone, then rne arrays (crb is dead by then) + qfrc parts
  l.u[U_crb] = 0;
  if (10 * nb > U) U = 10 * nb;
  off = 0;
  for (int k = U_cvel; k <= U_qfrc_actuator; k++) { l.u[k] = off; off += us[k]; }
  if (off > U) U = off;
  // constraints + solver
  off = 0;
  l.u[U_G] = off; off += us[U_G];
  l.u[U_aref] = off; off += us[U_aref];
  l.u[U_vel] = off; l.u[U_pos] = off + ne; l.u[U_margin] = off + 2 * ne; l.u[U_nH] = off; off += xreg;
  for (int k = U_scratch; k <= U_ndir; k++) { l.u[k] = off; off += us[k]; }
  if (off > U) U = off;
  // integration: M - dt qDeriv is formed in place in M (the qDeriv view is
  // not stored)
  l.u[U_qDeriv] = 0;
  sizes[L_U] = U;
  sizes[L_ints] = (16 + 3 * nc + 4 * ne + 1) / 2;
  off = 0;
  for (int k = 0; k < L_COUNT; k++) {
    l.o[k] = off;
    off += sizes[k];
  }
  l.ncon_max = nc;
  l.nefc_max = ne;
  l.nv = nv;
  l.total_doubles = off;
  *bytes = (size_t)off * sizeof(double);
  return l;
}

// a layout as the words mgs_model_layout exports and a specialised code object
// bakes: o[], u[], ncon_max, nefc_max, nv, total_doubles
constexpr int LAYOUT_WORDS = L_COUNT + U_COUNT + 4;
void layout_words(const Lay& l, int32_t* w) {
  int k = 0;
  for (int i = 0; i < L_COUNT; i++) w[k++] = l.o[i];
  for (int i = 0; i < U_COUNT; i++) w[k++] = l.u[i];
  w[k++] = l.ncon_max; w[k++] = l.nefc_max; w[k++] = l.nv; w[k++] = l.total_doubles;
}
}  // namespace

// dof counts with a compiled kernel instantiation (mgs_inst.hip, one translation
// unit each).  Main library: Panda + free object = 14, Robotiq 2F-85 + free
// object = 20, Allegro + free object = 28, Shadow + free object = 34.  Wide
// library (MGS_WIDE: 4 rows per lane, G in HBM) for clutter piles of 5 free
// objects: Panda 38, Robotiq 44, Allegro 52, Shadow 58.  Any other dof count
// (up to 64) runs through a model-specialised code object
// (mgs_model_attach_special).  The list is MGS_NV_LIST from the build
// (__graft_entry__.py), here the default.
#ifndef MGS_NV_LIST
#ifdef MGS_WIDE
#define MGS_NV_LIST(X) X(38) X(44) X(52) X(58)
#else
#define MGS_NV_LIST(X) X(14) X(20) X(28) X(34)
#endif
#endif

#define MGS_DECL(NV_) template <> const KernelSet* mgs_kernels_nv<NV_>();
MGS_NV_LIST(MGS_DECL)
#undef MGS_DECL

static const KernelSet* kernels_for(int nv) {
  switch (nv) {
#define MGS_CASE(NV_) case NV_: return mgs_kernels_nv<NV_>();
    MGS_NV_LIST(MGS_CASE)
#undef MGS_CASE
    default: return nullptr;
  }
}

static bool nv_supported(int nv) { return kernels_for(nv) != nullptr; }

// static LDS of the kernels (the diagnostic stage timers of the MGS_PROFILE build)
#ifdef MGS_PROFILE
#define MGS_STATIC_LDS (65 * 8)
#else
#define MGS_STATIC_LDS 0
#endif

static hipError_t set_lds_limit(int nv, int bytes) {
  const KernelSet* k = kernels_for(nv);
  if (!k) return hipSuccess;     // specialised-only dof count: nothing to set here
  hipError_t e = hipFuncSetAttribute(k->rollout_fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) return e;
  return hipFuncSetAttribute(k->collision_fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

struct mgs_model {
  mgs_model_desc desc;
  int device;
  int32_t* dI;
  double* dD;
  Lay lay;
  size_t lds_bytes;
  // model-specialised code object (mgs_special.hip), if attached
  hipModule_t special_mod;
  hipFunction_t special_collision, special_rollout;
  int resident;     // rollout workgroups the device holds at once (work-queue grid), 0 = not computed yet
};

struct mgs_batch {
  mgs_model* m;
  int cap;
  double *d_qpos, *d_mpos, *d_mquat, *d_ps, *d_pt, *d_objq;
  uint8_t *d_label, *d_free;
  int32_t *d_fail, *d_stats;
  double* d_G;      // MGS_G_GLOBAL: per-candidate constraint rows (HBM)
  size_t g_elems;
  double* d_resume; // resume records (n * (nq + 2 nv + nact + MGS_RESUME_EXTRA)), allocated on first use
  uint32_t* d_queue;                // work-queue headers (MGS_QHDR words: next index, exits, rotation
  int qslot;                        // ring head / tail, ring address), one per launch in a ring of
                                    // MGS_QUEUE_RING (launches in flight on other streams keep their
                                    // own); each launch's last workgroup returns its counters to zero
                                    // (the enough_stable count of ABI 24, word MGS_QSTABLE, included)
  uint32_t* d_rings;                // rotation rings (ABI 19), MGS_QRING_F(ring_n) words per header,
  int ring_n;                       // allocated on the first launch with yield_every > 0 and grown
                                    // when a launch's n exceeds ring_n (the kernel indexes a ring by
                                    // its launch's n, which may exceed the batch capacity: ADVICE r4)
  int qslot_drained;                // qslot at the last mgs_queue_spans (spans older than 64 launches are lost)
  uint64_t spins_seen;              // expired ring spins already reported (mgs_queue_stats word 7)
  hipEvent_t e0, e1, e2, e3;
  double last_ms;
};

extern "C" {

int mgs_abi_version(void) { return MGS_ABI_VERSION; }
const char* mgs_last_error(void) { return g_err.c_str(); }

int mgs_model_create(const mgs_model_desc* desc, const int32_t* ibuf, const double* dbuf, int device,
                     mgs_model** out) {
  if (!desc || !ibuf || !dbuf || !out) return fail(MGS_EINVAL, "mgs_model_create: null argument%s");
  if (desc->nv < 1) return fail(MGS_EINVAL, "nv must be >= 1%s");
  if (desc->cone != 1 || desc->integrator != 2)
    return fail(MGS_EINVAL, "only elliptic cones and implicitfast are supported%s");
  if (desc->nu > 32) return fail(MGS_EINVAL, "at most 32 actuators%s");
  if (desc->nmocap > 1) return fail(MGS_EINVAL, "at most one mocap body%s");
  if (desc->nefc_max > 64 * MGS_RPL) return fail(MGS_EINVAL, "nefc_max exceeds this library's rows (mgs_max_rows)%s");
  // more than 64 dofs: the model's specialised code object runs it (two dofs
  // per lane); the library's kernels refuse it at launch (no instantiation)
  if (desc->nv > MGS_MAX_NV) return fail(MGS_EINVAL, "nv must be <= 128 (two dofs per lane)%s");
  if (desc->nbody > 64) return fail(MGS_EINVAL, "at most 64 bodies (lanes over bodies)%s");
  if (desc->njnt > 64) return fail(MGS_EINVAL, "at most 64 joints (lanes over joints)%s");
  if (desc->maxcondim != 1 && desc->maxcondim != 3 && desc->maxcondim != 4 && desc->maxcondim != 6)
    return fail(MGS_EINVAL, "maxcondim must be 1, 3, 4 or 6%s");
  for (int p = 0; p < desc->npair; p++) {
    int cd = ibuf[desc->i_pair_condim + p];
    if (cd != 1 && cd != 3 && cd != 4 && cd != 6) return fail(MGS_EINVAL, "condim must be 1, 3, 4 or 6%s");
    if (cd > desc->maxcondim) return fail(MGS_EINVAL, "a pair's condim exceeds maxcondim%s");
  }
  if (desc->nact < 0 || desc->nact > 4 * 32) return fail(MGS_EINVAL, "bad nact%s");
  for (int u = 0, used = 0; u < desc->nu; u++) {
    const int adr = ibuf[desc->i_actuator_actadr + u];
    int need = 0;
    if (ibuf[desc->i_actuator_gaintype + u] == MGS_GAIN_PID) {
      const double* pp = dbuf + desc->d_actuator_pidprm + 5 * u;
      need = (pp[4] >= 0.0) + (pp[1] != 0.0);
    }
    if (need == 0 ? adr != -1 : adr != used)
      return fail(MGS_EINVAL, "actuator_actadr: a mujoco.pid actuator's act entries are its slew and integral "
                              "states, packed in actuator order%s");
    used += need;
    if (u == desc->nu - 1 && used != desc->nact) return fail(MGS_EINVAL, "nact differs from the actuators' act entries%s");
  }
  if (desc->nu == 0 && desc->nact != 0) return fail(MGS_EINVAL, "nact without actuators%s");
  HIPCHK(hipSetDevice(device));
  // (every member null: an early return frees what has been allocated by then)
  std::unique_ptr<mgs_model, void (*)(mgs_model*)> m(new mgs_model(), mgs_model_free);
  m->desc = *desc;
  m->device = device;
  size_t ib = sizeof(int32_t) * (desc->isize > 0 ? desc->isize : 1);
  size_t db = sizeof(double) * (desc->dsize > 0 ? desc->dsize : 1);
  if (hipMalloc(&m->dI, ib) != hipSuccess || hipMalloc(&m->dD, db) != hipSuccess)
    return fail(MGS_ENOMEM, "device allocation failed%s");
  HIPCHK(hipMemcpy(m->dI, ibuf, sizeof(int32_t) * desc->isize, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(m->dD, dbuf, sizeof(double) * desc->dsize, hipMemcpyHostToDevice));
  m->lay = make_layout(*desc, &m->lds_bytes);
  if (m->lds_bytes > 160 * 1024 - MGS_STATIC_LDS) {
    char buf[64];
    snprintf(buf, sizeof(buf), "%zu", m->lds_bytes);
    return fail(MGS_ECAPACITY, "per-candidate working set %s B exceeds 160 KiB LDS; lower ncon_max", buf);
  }
  // the attribute is per kernel function, shared by every model of this nv: set it
  // to the CU's whole LDS so a later, smaller model cannot lower it under an
  // earlier, wider one (occupancy follows each launch's own dynamic size)
  HIPCHK(set_lds_limit(desc->nv, 160 * 1024 - MGS_STATIC_LDS));
  *out = m.release();
  return MGS_OK;
}

void mgs_model_free(mgs_model* m) {
  if (!m) return;
  if (m->special_mod) hipModuleUnload(m->special_mod);
  hipFree(m->dI);     // (null when mgs_model_create failed before it: hipFree(nullptr) is a no-op)
  hipFree(m->dD);
  delete m;
}

int mgs_batch_open(mgs_model* model, int capacity, mgs_batch** out) {
  if (!model || capacity <= 0 || !out) return fail(MGS_EINVAL, "mgs_batch_open: bad argument%s");
  HIPCHK(hipSetDevice(model->device));
  std::unique_ptr<mgs_batch, void (*)(mgs_batch*)> b(new mgs_batch(), mgs_batch_close);
  b->m = model;
  b->cap = capacity;
  const mgs_model_desc& d = model->desc;
  size_t n = (size_t)capacity;
  bool ok = hipMalloc(&b->d_qpos, sizeof(double) * n * d.nq) == hipSuccess &&
            hipMalloc(&b->d_mpos, sizeof(double) * n * 3) == hipSuccess &&
            hipMalloc(&b->d_mquat, sizeof(double) * n * 4) == hipSuccess &&
            hipMalloc(&b->d_ps, sizeof(double) * n * 3 * MGS_MAX_PHASES) == hipSuccess &&
            hipMalloc(&b->d_pt, sizeof(double) * n * 3 * MGS_MAX_PHASES) == hipSuccess &&
            hipMalloc(&b->d_objq, sizeof(double) * n * 7) == hipSuccess &&
            hipMalloc(&b->d_label, n) == hipSuccess && hipMalloc(&b->d_free, n) == hipSuccess &&
            hipMalloc(&b->d_fail, sizeof(int32_t) * n) == hipSuccess &&
            hipMalloc(&b->d_stats, sizeof(int32_t) * n * MGS_NSTATS) == hipSuccess &&
            hipMalloc(&b->d_queue, MGS_QHDR * sizeof(uint32_t) * MGS_QUEUE_RING) == hipSuccess &&
            hipMemset(b->d_queue, 0, MGS_QHDR * sizeof(uint32_t) * MGS_QUEUE_RING) == hipSuccess &&
            // the counters must be zero before any stream's launch reads them
            // (hipMemset may still be in flight on the null stream otherwise)
            hipDeviceSynchronize() == hipSuccess;
  if (!ok) return fail(MGS_ENOMEM, "device allocation failed%s");
  HIPCHK(hipEventCreate(&b->e0));
  HIPCHK(hipEventCreate(&b->e1));
  HIPCHK(hipEventCreate(&b->e2));
  HIPCHK(hipEventCreate(&b->e3));
  *out = b.release();
  return MGS_OK;
}

void mgs_batch_close(mgs_batch* b) {
  if (!b) return;
  hipFree(b->d_qpos); hipFree(b->d_mpos); hipFree(b->d_mquat); hipFree(b->d_ps); hipFree(b->d_pt);
  hipFree(b->d_objq); hipFree(b->d_label); hipFree(b->d_free); hipFree(b->d_fail); hipFree(b->d_stats);
  if (b->d_G) hipFree(b->d_G);
  if (b->d_resume) hipFree(b->d_resume);
  if (b->d_queue) hipFree(b->d_queue);
  if (b->d_rings) hipFree(b->d_rings);
  if (b->e0) hipEventDestroy(b->e0);
  if (b->e1) hipEventDestroy(b->e1);
  if (b->e2) hipEventDestroy(b->e2);
  if (b->e3) hipEventDestroy(b->e3);
  delete b;
}

// the layout a launch over n candidates uses: in the wide library the G rows of
// every candidate live in a batch-owned HBM buffer, grown on demand
static int launch_layout(mgs_batch* b, int n, Lay* lay) {
  *lay = b->m->lay;
  lay->gmem = nullptr;
  if (g_in_hbm(b->m->desc)) {
    size_t need = (size_t)n * hbm_slice_doubles(b->m->desc);
    if (need > b->g_elems) {
      if (b->d_G) HIPCHK(hipFree(b->d_G));
      b->d_G = nullptr;
      b->g_elems = 0;
      if (hipMalloc(&b->d_G, need * sizeof(double)) != hipSuccess)
        return fail(MGS_ENOMEM, "G buffer allocation failed%s");
      b->g_elems = need;
    }
    lay->gmem = b->d_G;
  }
  return MGS_OK;
}

// Rollout launches run as a work queue by default: the grid is the number of
// rollout workgroups the device holds at once (occupancy of the launched
// function at this model's LDS size x CUs) and each workgroup pulls candidate
// indices from a counter (reset by the launch's last workgroup, see rollout_entry).  Mode (mgs_rollout_queue; MGS_QUEUE in the
// environment sets the initial one): 0 one workgroup per candidate, 1 the
// queue on the resident grid, k >= 2 the queue on at most k workgroups (tests).
static int g_queue_mode = -1;

static int queue_mode() {
  if (g_queue_mode < 0) {
    const char* e = getenv("MGS_QUEUE");
    g_queue_mode = e ? atoi(e) : 1;
    if (g_queue_mode < 0) g_queue_mode = 1;
  }
  return g_queue_mode;
}

static int resident_workgroups(mgs_model* m) {
  if (m->resident) return m->resident;
  int per_cu = 0, cus = 0;
  hipError_t e;
  if (m->special_rollout) {
    e = hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, m->special_rollout, 64, m->lds_bytes);
  } else {
    const KernelSet* k = kernels_for(m->desc.nv);
    e = k ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k->rollout_fn, 64, m->lds_bytes) : hipErrorInvalidValue;
  }
  if (e != hipSuccess || per_cu < 1 ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, m->device) != hipSuccess || cus < 1) {
    (void)hipGetLastError();
    m->resident = -1;       // unknown: one workgroup per candidate
    return -1;
  }
  m->resident = per_cu * cus;
  return m->resident;
}

// the grid rule: a launch over n candidates runs as a work queue on the
// resident workgroups (at most k of them in mode k >= 2) when those are fewer
// than n; 0 = one workgroup per candidate, no queue
static int queue_grid(mgs_model* m, int n) {
  if (queue_mode() == 0) return 0;
  int r = resident_workgroups(m);
  if (queue_mode() > 1 && r > queue_mode()) r = queue_mode();
  return (r > 0 && r < n) ? r : 0;
}

int mgs_model_resident(mgs_model* model) {
  if (!model) return fail(MGS_EINVAL, "mgs_model_resident: null model%s");
  HIPCHK(hipSetDevice(model->device));
  return resident_workgroups(model);
}

static Mdl device_model(const mgs_model* m) {
  Mdl md;
  md.m = m->desc;
  md.I = m->dI;
  md.D = m->dD;
  return md;
}

int mgs_collision_free_device(mgs_batch* b, int n, const double* d_qpos_init, const double* d_mocap_pos,
                              const double* d_mocap_quat, int predicate, uint8_t* d_out_free, void* stream) {
  if (!b || n < 0) return fail(MGS_EINVAL, "mgs_collision_free_device: bad argument%s");
  if (n == 0) return MGS_OK;
  if (!d_qpos_init || !d_mocap_pos || !d_mocap_quat || !d_out_free) return fail(MGS_EINVAL, "null argument%s");
  if (predicate != MGS_PRED_ANY_CONTACT && predicate != MGS_PRED_PARTITION && predicate != MGS_PRED_PARTITION_INCL)
    return fail(MGS_EINVAL, "unknown contact predicate%s");
  HIPCHK(hipSetDevice(b->m->device));
  hipStream_t st = (hipStream_t)stream;
  Mdl md = device_model(b->m);
  Lay lay;
  int lrc = launch_layout(b, n, &lay);
  if (lrc) return lrc;
  HIPCHK(hipEventRecord(b->e2, st));
  CollisionArgs a{md, lay, n, d_qpos_init, d_mocap_pos, d_mocap_quat, predicate, d_out_free};
  if (b->m->special_collision) {
    const int32_t* I = md.I;
    const double* D = md.D;
    void* p[] = {&a.md, &I, &D, &a.lay, &a.n, &a.qpos_init, &a.mocap_pos, &a.mocap_quat, &a.predicate, &a.out};
    HIPCHK(hipModuleLaunchKernel(b->m->special_collision, n, 1, 1, 64, 1, 1, b->m->lds_bytes, st, p, nullptr));
  } else {
    const KernelSet* k = kernels_for(md.m.nv);
    if (!k) return fail(MGS_EINVAL, "no kernel for this nv in this library and no specialised code object attached%s");
    k->collision(dim3(n), b->m->lds_bytes, st, a);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(b->e3, st));
  return MGS_OK;
}

int mgs_collision_free(mgs_batch* b, int n, const double* qpos_init, const double* mocap_pos,
                       const double* mocap_quat, int predicate, uint8_t* out_free) {
  if (!b || n < 0 || n > b->cap) return fail(MGS_EINVAL, "mgs_collision_free: n exceeds batch capacity%s");
  if (n == 0) return MGS_OK;
  if (!qpos_init || !mocap_pos || !mocap_quat || !out_free) return fail(MGS_EINVAL, "null argument%s");
  const mgs_model_desc& d = b->m->desc;
  HIPCHK(hipSetDevice(b->m->device));
  HIPCHK(hipMemcpy(b->d_qpos, qpos_init, sizeof(double) * n * d.nq, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->d_mpos, mocap_pos, sizeof(double) * n * 3, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->d_mquat, mocap_quat, sizeof(double) * n * 4, hipMemcpyHostToDevice));
  int rc = mgs_collision_free_device(b, n, b->d_qpos, b->d_mpos, b->d_mquat, predicate, b->d_free, nullptr);
  if (rc) return rc;
  HIPCHK(hipMemcpy(out_free, b->d_free, n, hipMemcpyDeviceToHost));
  return MGS_OK;
}

// the rotation rings of every queue header for launches of up to n
// candidates (zeroed; each header's words 4-5 get its ring's address; a
// launch over n indexes MGS_QRING_F(n) words of its ring).  Synchronous: on
// the first rotating launch, and again whenever a launch's n exceeds the n the
// rings were sized for (the old rings are freed once no launch uses them).
static int alloc_rings(mgs_batch* b, int n) {
  if (b->d_rings && b->ring_n >= n) return MGS_OK;
  const size_t per = MGS_QRING_F(n);
  HIPCHK(hipDeviceSynchronize());   // no launch holds a header or a ring while they are replaced
  if (b->d_rings) {
    HIPCHK(hipFree(b->d_rings));
    b->d_rings = nullptr;
    b->ring_n = 0;
  }
  if (hipMalloc(&b->d_rings, sizeof(uint32_t) * per * MGS_QUEUE_RING) != hipSuccess) {
    b->d_rings = nullptr;
    uint64_t z = 0;
    for (int k = 0; k < MGS_QUEUE_RING; k++)      // no header may point at the freed rings
      HIPCHK(hipMemcpy(b->d_queue + MGS_QHDR * k + 4, &z, sizeof(z), hipMemcpyHostToDevice));
    return fail(MGS_ENOMEM, "rotation ring allocation failed%s");
  }
  HIPCHK(hipMemset(b->d_rings, 0, sizeof(uint32_t) * per * MGS_QUEUE_RING));
  for (int k = 0; k < MGS_QUEUE_RING; k++) {
    uint64_t a = (uint64_t)(uintptr_t)(b->d_rings + per * k);
    HIPCHK(hipMemcpy(b->d_queue + MGS_QHDR * k + 4, &a, sizeof(a), hipMemcpyHostToDevice));
  }
  HIPCHK(hipDeviceSynchronize());
  b->ring_n = n;
  return MGS_OK;
}

// every queue header of a batch, once the device is idle
static int read_queue_headers(mgs_batch* b, uint32_t (&h)[MGS_QHDR * MGS_QUEUE_RING]) {
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(h, b->d_queue, sizeof(h), hipMemcpyDeviceToHost));
  return MGS_OK;
}

// the expired-spin counters (word 7 of every queue header), summed
static int expired_spins(mgs_batch* b, uint64_t* out) {
  uint32_t h[MGS_QHDR * MGS_QUEUE_RING];
  int rc = read_queue_headers(b, h);
  if (rc) return rc;
  uint64_t e = 0;
  for (int k = 0; k < MGS_QUEUE_RING; k++) e += h[MGS_QHDR * k + 7];
  *out = e;
  return MGS_OK;
}

// ring spins expired since the last look (a candidate possibly lost, a ring
// slot possibly written after its launch ended) are acknowledged and every
// ring and ring head / tail is reset, so the next launch starts from a clean
// protocol state; *expired (optional) tells whether there were any
static int reset_expired(mgs_batch* b, bool* expired = nullptr) {
  if (expired) *expired = false;
  if (!b->d_rings) return MGS_OK;
  uint64_t e = 0;
  int rc = expired_spins(b, &e);
  if (rc) return rc;
  if (e == b->spins_seen) return MGS_OK;
  if (expired) *expired = true;
  b->spins_seen = e;
  HIPCHK(hipMemset(b->d_rings, 0, sizeof(uint32_t) * MGS_QRING_F(b->ring_n) * MGS_QUEUE_RING));
  for (int k = 0; k < MGS_QUEUE_RING; k++)
    HIPCHK(hipMemset(b->d_queue + MGS_QHDR * k + 2, 0, 2 * sizeof(uint32_t)));
  HIPCHK(hipDeviceSynchronize());
  return MGS_OK;
}

// after a rotating launch of a synchronous entry: an expired ring spin fails
// the call with MGS_EQUEUE
static int check_rotation(mgs_batch* b) {
  bool expired;
  int rc = reset_expired(b, &expired);
  if (rc || !expired) return rc;
  return fail(MGS_EQUEUE, "rotation ring protocol timed out (expired spin): a candidate may have been lost; "
                          "the launch's outputs are invalid%s");
}

// one rollout launch.  The caller names what it uses of `a` (n, the candidates'
// inputs and outputs, the list, resume records, fused mask, overflow header);
// md, lay, sc, queue and ovf_list are filled here.  A launch over a list runs
// list_grid workgroups, any other the grid rule's.
static int launch_rollout(mgs_batch* b, const mgs_schedule* sched, RolloutArgs a, void* stream, int list_grid = 0) {
  if (!b || !sched || a.n < 0) return fail(MGS_EINVAL, "mgs_rollout_device: bad argument%s");
  if (sched->nphase < 1 || sched->nphase > MGS_MAX_PHASES) return fail(MGS_EINVAL, "bad phase count%s");
  if (a.n == 0) return MGS_OK;
  HIPCHK(hipSetDevice(b->m->device));
  hipStream_t st = (hipStream_t)stream;
  a.md = device_model(b->m);
  a.sc = *sched;
  a.queue = nullptr;
  a.ovf_list = a.ovf_count ? a.ovf_count + MGS_LIST_HEADER : nullptr;
  int nwg = a.list ? list_grid : a.n;
  if (const int r = a.list ? 0 : queue_grid(b->m, a.n)) {
    nwg = r;
    a.queue = b->d_queue + MGS_QHDR * (b->qslot++ % MGS_QUEUE_RING);
    if (sched->yield_every > 0 && a.resume_out) {
      int rrc = alloc_rings(b, a.n);
      if (rrc) return rrc;
    }
  }
  int lrc = launch_layout(b, nwg, &a.lay);
  if (lrc) return lrc;
  HIPCHK(hipEventRecord(b->e0, st));
  const Mdl& md = a.md;
  if (b->m->special_rollout) {
    const int32_t* I = md.I;
    const double* D = md.D;
    void* p[] = {&a.md, &I, &D, &a.lay, &a.sc, &a.n, &a.qpos_init, &a.mocap_quat, &a.phase_start, &a.phase_target,
                 &a.active, &a.label, &a.fail_step, &a.obj_qpos, &a.stats, &a.vstate_init, &a.state_out, &a.list,
                 &a.list_count, &a.resume_out, &a.resume_in, &a.mask_mpos, &a.mask_pred, &a.mask_out, &a.queue,
                 &a.ovf_count, &a.ovf_list};
    HIPCHK(hipModuleLaunchKernel(b->m->special_rollout, nwg, 1, 1, 64, 1, 1, b->m->lds_bytes, st, p, nullptr));
  } else {
    const KernelSet* k = kernels_for(md.m.nv);
    if (!k) return fail(MGS_EINVAL, "no kernel for this nv in this library and no specialised code object attached%s");
    if (layout_maxdim(md.m) > MGS_MAXDIM)
      return fail(MGS_EINVAL, "condim-6 contacts run through the model's specialised code object only "
                              "(mgs.core.special); none is attached%s");
#ifndef MGS_G_GLOBAL
    if (md.m.g_rows_hbm)
      return fail(MGS_EINVAL, "g_rows_hbm: G rows in HBM need the model's specialised code object%s");
#endif
    k->rollout(dim3(nwg), b->m->lds_bytes, st, a);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(b->e1, st));
  return MGS_OK;
}

int mgs_rollout_device(mgs_batch* b, const mgs_schedule* sched, int n, const double* d_qpos_init,
                       const double* d_mocap_quat, const double* d_phase_start, const double* d_phase_target,
                       const uint8_t* d_active, uint8_t* d_label, int32_t* d_fail_step, double* d_obj_qpos,
                       int32_t* d_stats, void* stream) {
  RolloutArgs a{};
  a.n = n; a.qpos_init = d_qpos_init; a.mocap_quat = d_mocap_quat;
  a.phase_start = d_phase_start; a.phase_target = d_phase_target; a.active = d_active;
  a.label = d_label; a.fail_step = d_fail_step; a.obj_qpos = d_obj_qpos; a.stats = d_stats;
  return launch_rollout(b, sched, a, stream);
}

int mgs_queue_stats(mgs_batch* b, uint64_t* out) {
  if (!b || !out) return fail(MGS_EINVAL, "mgs_queue_stats: null argument%s");
  HIPCHK(hipSetDevice(b->m->device));
  uint32_t h[MGS_QHDR * MGS_QUEUE_RING];
  int rc = read_queue_headers(b, h);
  if (rc) return rc;
  out[0] = out[1] = 0;
  for (int k = 0; k < MGS_QUEUE_RING; k++) {
    out[0] += h[MGS_QHDR * k + 6];
    out[1] += h[MGS_QHDR * k + 7];
  }
  return MGS_OK;
}

int mgs_queue_spans(mgs_batch* b, double* out_ms, int cap, int* count, int* overwritten) {
  if (!b || !out_ms || !count || cap < 0) return fail(MGS_EINVAL, "mgs_queue_spans: bad argument%s");
  // launches since the previous call beyond the ring's 64 headers: their spans
  // were overwritten before they could be read
  const int since = b->qslot - b->qslot_drained;
  if (overwritten) *overwritten = since > MGS_QUEUE_RING ? since - MGS_QUEUE_RING : 0;
  b->qslot_drained = b->qslot;
  HIPCHK(hipSetDevice(b->m->device));
  uint32_t h[MGS_QHDR * MGS_QUEUE_RING];
  int rc = read_queue_headers(b, h);
  if (rc) return rc;
  int k = 0;
  for (int i = 0; i < MGS_QUEUE_RING; i++) {
    // oldest first: the slot after the last one handed out
    const int s = (b->qslot + i) % MGS_QUEUE_RING;
    uint64_t t0, t1;
    memcpy(&t0, h + MGS_QHDR * s + 8, sizeof(t0));
    memcpy(&t1, h + MGS_QHDR * s + 10, sizeof(t1));
    if (t0 == 0 || t1 <= t0) continue;
    if (k < cap) out_ms[k++] = (double)(t1 - t0) * 1e-5;   // 100 MHz ticks
    HIPCHK(hipMemset(b->d_queue + MGS_QHDR * s + 8, 0, 4 * sizeof(uint32_t)));
  }
  HIPCHK(hipDeviceSynchronize());
  *count = k;
  return MGS_OK;
}

int mgs_overflow_list_device(int n, const int32_t* d_stats, int flag_mask, int32_t* d_count, int32_t* d_list,
                             void* stream) {
  if (n < 0 || !d_stats || !d_count || !d_list) return fail(MGS_EINVAL, "mgs_overflow_list_device: bad argument%s");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(d_count, 0, 2 * sizeof(int32_t), st));   // count and exits of the list header
  if (n == 0) return MGS_OK;
  hipLaunchKernelGGL(mgs_overflow_list_kernel, dim3((n + 255) / 256), dim3(256), 0, st, d_stats, n, flag_mask, d_count,
                     d_list);
  HIPCHK(hipGetLastError());
  return MGS_OK;
}

int mgs_rollout_list_device(mgs_batch* b, const mgs_schedule* sched, int n, int32_t* d_count,
                            const int32_t* d_list, int grid, const double* d_qpos_init, const double* d_mocap_quat,
                            const double* d_phase_start, const double* d_phase_target, const double* d_resume_in,
                            uint8_t* d_label, int32_t* d_fail_step, double* d_obj_qpos, int32_t* d_stats,
                            void* stream) {
  if (!b || !d_count || !d_list || grid < 1 || grid > b->cap)
    return fail(MGS_EINVAL, "mgs_rollout_list_device: bad argument (1 <= grid <= batch capacity)%s");
  RolloutArgs a{};
  a.n = n; a.qpos_init = d_qpos_init; a.mocap_quat = d_mocap_quat;
  a.phase_start = d_phase_start; a.phase_target = d_phase_target;
  a.label = d_label; a.fail_step = d_fail_step; a.obj_qpos = d_obj_qpos; a.stats = d_stats;
  a.list = d_list; a.list_count = d_count; a.resume_in = d_resume_in;
  return launch_rollout(b, sched, a, stream, grid);
}

int mgs_rollout_resumable_device(mgs_batch* b, const mgs_schedule* sched, int n, const double* d_qpos_init,
                                 const double* d_mocap_quat, const double* d_phase_start,
                                 const double* d_phase_target, const uint8_t* d_active, uint8_t* d_label,
                                 int32_t* d_fail_step, double* d_obj_qpos, int32_t* d_stats, double* d_resume_out,
                                 int32_t* d_ovf, void* stream) {
  if (!d_resume_out) return fail(MGS_EINVAL, "mgs_rollout_resumable_device: null resume buffer%s");
  RolloutArgs a{};
  a.n = n; a.qpos_init = d_qpos_init; a.mocap_quat = d_mocap_quat;
  a.phase_start = d_phase_start; a.phase_target = d_phase_target; a.active = d_active;
  a.label = d_label; a.fail_step = d_fail_step; a.obj_qpos = d_obj_qpos; a.stats = d_stats;
  a.resume_out = d_resume_out; a.ovf_count = d_ovf;
  return launch_rollout(b, sched, a, stream);
}

int mgs_mask_rollout_device(mgs_batch* b, const mgs_schedule* sched, int n, const double* d_qpos_init,
                            const double* d_mocap_pos, const double* d_mocap_quat, const double* d_phase_start,
                            const double* d_phase_target, int predicate, uint8_t* d_free_out, uint8_t* d_label,
                            int32_t* d_fail_step, double* d_obj_qpos, int32_t* d_stats, double* d_resume_out,
                            int32_t* d_ovf, void* stream) {
  if (!d_mocap_pos || !d_free_out) return fail(MGS_EINVAL, "mgs_mask_rollout_device: mocap_pos and free_out are required%s");
  if (predicate < MGS_PRED_ANY_CONTACT || predicate > MGS_PRED_PARTITION_INCL)
    return fail(MGS_EINVAL, "mgs_mask_rollout_device: bad predicate%s");
  RolloutArgs a{};
  a.n = n; a.qpos_init = d_qpos_init; a.mocap_quat = d_mocap_quat;
  a.phase_start = d_phase_start; a.phase_target = d_phase_target;
  a.label = d_label; a.fail_step = d_fail_step; a.obj_qpos = d_obj_qpos; a.stats = d_stats;
  a.resume_out = d_resume_out; a.ovf_count = d_ovf;
  a.mask_mpos = d_mocap_pos; a.mask_pred = predicate; a.mask_out = d_free_out;
  return launch_rollout(b, sched, a, stream);
}

int mgs_simulate_device(mgs_batch* b, const mgs_schedule* sched, int n, const double* d_qpos_init,
                        const double* d_vstate_init, const double* d_mocap_quat, const double* d_phase_start,
                        const double* d_phase_target, double* d_state_out, int32_t* d_stats, void* stream) {
  if (!b || !sched || !d_state_out || n < 0 || n > b->cap) return fail(MGS_EINVAL, "mgs_simulate_device: bad argument%s");
  mgs_schedule s = *sched;   // no contact checks: a free simulation never stops early
  for (int p = 0; p < MGS_MAX_PHASES; p++) { s.check_every[p] = 0; s.check_at_end[p] = 0; }
  s.enough_stable = 0;       // every state ends "ok" here: nothing to count, nothing to skip
  RolloutArgs a{};
  a.n = n; a.qpos_init = d_qpos_init; a.mocap_quat = d_mocap_quat;
  a.phase_start = d_phase_start; a.phase_target = d_phase_target;
  a.label = b->d_label; a.fail_step = b->d_fail; a.obj_qpos = b->d_objq; a.stats = d_stats ? d_stats : b->d_stats;
  a.vstate_init = d_vstate_init; a.state_out = d_state_out;
  return launch_rollout(b, &s, a, stream);
}

int mgs_simulate(mgs_batch* b, const mgs_schedule* sched, int n, const double* qpos_init,
                 const double* vstate_init, const double* mocap_quat, const double* phase_start,
                 const double* phase_target, double* state_out, int32_t* stats) {
  if (!b || !sched || n < 0 || n > b->cap) return fail(MGS_EINVAL, "mgs_simulate: bad argument%s");
  if (n == 0) return MGS_OK;
  if (!qpos_init || !mocap_quat || !phase_start || !phase_target || !state_out)
    return fail(MGS_EINVAL, "mgs_simulate: null argument%s");
  const mgs_model_desc& d = b->m->desc;
  int np = sched->nphase;
  HIPCHK(hipSetDevice(b->m->device));
  const size_t nst = (size_t)n * (d.nq + 2 * d.nv + d.nact);
  DevBufs bufs;
  double* ds = bufs.get<double>(nst);
  double* dv = vstate_init ? upload(bufs, vstate_init, (size_t)n * (2 * d.nv + d.nact)) : nullptr;
  if (!bufs.ok) return fail(MGS_ENOMEM, "state buffer allocation or upload failed%s");
  HIPCHK(hipMemcpy(b->d_qpos, qpos_init, sizeof(double) * n * d.nq, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->d_mquat, mocap_quat, sizeof(double) * n * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->d_ps, phase_start, sizeof(double) * n * 3 * np, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->d_pt, phase_target, sizeof(double) * n * 3 * np, hipMemcpyHostToDevice));
  int rc = mgs_simulate_device(b, sched, n, b->d_qpos, dv, b->d_mquat, b->d_ps, b->d_pt, ds, nullptr, nullptr);
  if (rc) return rc;
  HIPCHK(hipMemcpy(state_out, ds, nst * sizeof(double), hipMemcpyDeviceToHost));
  if (stats) HIPCHK(hipMemcpy(stats, b->d_stats, sizeof(int32_t) * n * MGS_NSTATS, hipMemcpyDeviceToHost));
  return MGS_OK;
}

double mgs_last_collision_ms(mgs_batch* b) {
  if (!b) return -1.0;
  float ms = 0.f;
  if (hipEventSynchronize(b->e3) != hipSuccess) return -1.0;
  if (hipEventElapsedTime(&ms, b->e2, b->e3) != hipSuccess) return -1.0;
  return ms;
}

double mgs_last_kernel_ms(mgs_batch* b) {
  if (!b) return -1.0;
  float ms = 0.f;
  if (hipEventSynchronize(b->e1) != hipSuccess) return -1.0;
  if (hipEventElapsedTime(&ms, b->e0, b->e1) != hipSuccess) return -1.0;
  b->last_ms = ms;
  return ms;
}

static int rollout_host(mgs_batch* b, const mgs_schedule* sched, int n, const double* qpos_init,
                        const double* mocap_quat, const double* phase_start, const double* phase_target,
                        const double* resume_in, mgs_rollout_out* out) {
  if (!b || !sched || !out || n < 0 || n > b->cap) return fail(MGS_EINVAL, "mgs_rollout: bad argument%s");
  if (n == 0) return MGS_OK;
  if (!qpos_init || !mocap_quat || !phase_start || !phase_target || !out->label)
    return fail(MGS_EINVAL, "mgs_rollout: null argument%s");
  const mgs_model_desc& d = b->m->desc;
  int np = sched->nphase;
  HIPCHK(hipSetDevice(b->m->device));
  const size_t rs = (size_t)d.nq + 2 * (size_t)d.nv + (size_t)d.nact + MGS_RESUME_EXTRA;
  // resume records: one buffer serves as the output of a resumable run or the
  // input of a resumed one
  if ((out->resume || resume_in) && !b->d_resume &&
      hipMalloc(&b->d_resume, sizeof(double) * rs * (size_t)b->cap) != hipSuccess)
    return fail(MGS_ENOMEM, "resume buffer allocation failed%s");
  HIPCHK(hipMemcpy(b->d_qpos, qpos_init, sizeof(double) * n * d.nq, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->d_mquat, mocap_quat, sizeof(double) * n * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->d_ps, phase_start, sizeof(double) * n * 3 * np, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->d_pt, phase_target, sizeof(double) * n * 3 * np, hipMemcpyHostToDevice));
  if (resume_in) HIPCHK(hipMemcpy(b->d_resume, resume_in, sizeof(double) * rs * n, hipMemcpyHostToDevice));
  int rc;
  // before a synchronous rotating launch: expired spins left by earlier launches
  // (the device entries', which their callers audit) are acknowledged here and
  // the rings they may have left dirty are reset, so the check after this launch
  // counts only its own
  if (sched->yield_every > 0 && (rc = reset_expired(b))) return rc;
  RolloutArgs a{};
  a.n = n; a.qpos_init = b->d_qpos; a.mocap_quat = b->d_mquat;
  a.phase_start = b->d_ps; a.phase_target = b->d_pt;
  a.label = b->d_label; a.fail_step = b->d_fail; a.obj_qpos = b->d_objq; a.stats = b->d_stats;
  a.resume_out = out->resume ? b->d_resume : nullptr;
  a.resume_in = resume_in ? b->d_resume : nullptr;
  rc = launch_rollout(b, sched, a, nullptr);
  if (rc) return rc;
  if (sched->yield_every > 0 && (rc = check_rotation(b))) return rc;
  HIPCHK(hipMemcpy(out->label, b->d_label, n, hipMemcpyDeviceToHost));
  if (out->fail_step) HIPCHK(hipMemcpy(out->fail_step, b->d_fail, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  if (out->obj_qpos) HIPCHK(hipMemcpy(out->obj_qpos, b->d_objq, sizeof(double) * n * 7, hipMemcpyDeviceToHost));
  if (out->stats) HIPCHK(hipMemcpy(out->stats, b->d_stats, sizeof(int32_t) * n * MGS_NSTATS, hipMemcpyDeviceToHost));
  if (out->resume) HIPCHK(hipMemcpy(out->resume, b->d_resume, sizeof(double) * rs * n, hipMemcpyDeviceToHost));
  return MGS_OK;
}

int mgs_rollout(mgs_batch* b, const mgs_schedule* sched, int n, const double* qpos_init,
                const double* mocap_quat, const double* phase_start, const double* phase_target,
                mgs_rollout_out* out) {
  return rollout_host(b, sched, n, qpos_init, mocap_quat, phase_start, phase_target, nullptr, out);
}

int mgs_rollout_resume(mgs_batch* b, const mgs_schedule* sched, int n, const double* qpos_init,
                       const double* mocap_quat, const double* phase_start, const double* phase_target,
                       const double* resume, mgs_rollout_out* out) {
  if (!resume) return fail(MGS_EINVAL, "mgs_rollout_resume: null resume records%s");
  return rollout_host(b, sched, n, qpos_init, mocap_quat, phase_start, phase_target, resume, out);
}

// test hook: device arithmetic on n inputs (out: n*4 = sqrt|x|, x/y, sin, cos)
int mgs_arith_probe(const double* x, const double* y, int n, double* out) {
  if (n < 0) return fail(MGS_EINVAL, "mgs_arith_probe: negative size%s");
  if (n == 0) return MGS_OK;
  if (!x || !y || !out) return fail(MGS_EINVAL, "mgs_arith_probe: null argument%s");
  DevBufs b;
  double* dx = upload(b, x, (size_t)n);
  double* dy = upload(b, y, (size_t)n);
  double* dout = b.get<double>(4 * (size_t)n);
  if (!b.ok) return fail(MGS_ENOMEM, "device allocation or upload failed%s");
  hipLaunchKernelGGL(mgs_arith_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, dx, dy, n, dout);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dout, sizeof(double) * n * 4, hipMemcpyDeviceToHost));
  return MGS_OK;
}

// test hook: pairwise-tree wave reduction, nb blocks of 64 lanes
int mgs_tree_probe(const double* a, const double* c, int n, int nb, double* out) {
  if (n < 0 || nb < 0) return fail(MGS_EINVAL, "mgs_tree_probe: negative size%s");
  if (nb == 0) return MGS_OK;
  if (!a || !c || !out) return fail(MGS_EINVAL, "mgs_tree_probe: null argument%s");
  DevBufs b;
  double* da = upload(b, a, 64 * (size_t)nb);
  double* dc = upload(b, c, 64 * (size_t)nb);
  double* dout = b.get<double>((size_t)nb);
  if (!b.ok) return fail(MGS_ENOMEM, "device allocation or upload failed%s");
  hipLaunchKernelGGL(mgs_tree_probe_kernel, dim3(nb), dim3(64), 0, 0, da, dc, n, dout);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dout, sizeof(double) * nb, hipMemcpyDeviceToHost));
  return MGS_OK;
}

// diagnostic build only: read and clear the stage timers (s_memtime ticks) of
// every dof count's kernels of this library
int mgs_prof_read(unsigned long long* out) {
#ifdef MGS_PROFILE
  for (int k = 0; k < 64; k++) out[k] = 0;
#define MGS_CASE(NV_) if (mgs_kernels_nv<NV_>()->prof_read(out)) return fail(MGS_EHIP, "stage timer read failed%s");
  MGS_NV_LIST(MGS_CASE)
#undef MGS_CASE
  return MGS_OK;
#else
  (void)out;
  return MGS_EINVAL;
#endif
}

// the same for a model's specialised code object (built with -DMGS_PROFILE)
int mgs_model_prof_read(mgs_model* m, unsigned long long* out) {
  if (!m || !m->special_mod || !out) return fail(MGS_EINVAL, "mgs_model_prof_read: no specialised code object%s");
  hipDeviceptr_t p;
  size_t sz = 0;
  unsigned long long z[64] = {0};
  if (hipModuleGetGlobal(&p, &sz, m->special_mod, "g_prof") != hipSuccess || sz != sizeof(z))
    return fail(MGS_EINVAL, "the specialised code object has no stage timers (not an MGS_PROFILE build)%s");
  HIPCHK(hipMemcpyDtoH(out, p, sizeof(z)));
  HIPCHK(hipMemcpyHtoD(p, z, sizeof(z)));
  return MGS_OK;
}

int mgs_lds_bytes(mgs_model* m) { return m ? (int)m->lds_bytes : -1; }

int mgs_antipodal_contacts(int device, const double* tri, int ntri, int n, const double* origin,
                           const double* dir, const double* u_choice, double eps, double* out_second,
                           int32_t* out_nvalid, double* kernel_ms) {
  if (n < 0 || ntri < 0) return fail(MGS_EINVAL, "mgs_antipodal_contacts: negative size%s");
  if (n == 0) return MGS_OK;
  if (!tri || !origin || !dir || !u_choice || !out_second || !out_nvalid)
    return fail(MGS_EINVAL, "mgs_antipodal_contacts: null argument%s");
  HIPCHK(hipSetDevice(device));
  const size_t nn = (size_t)n;
  DevBufs b;
  double* dT = upload(b, tri, 9 * (size_t)ntri);
  double* dO = upload(b, origin, 3 * nn);
  double* dD = upload(b, dir, 3 * nn);
  double* dU = upload(b, u_choice, nn);
  double* dS = b.get<double>(3 * nn);
  int32_t* dN = b.get<int32_t>(nn);
  if (!b.ok) return fail(MGS_ENOMEM, "device allocation or upload failed%s");
  EvTimer t;
  hipLaunchKernelGGL(mgs_antipodal_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, dT, ntri, n, dO, dD, dU,
                     eps, dS, dN);
  int rc = t.finish(kernel_ms);
  if (rc == MGS_OK) {
    HIPCHK(hipMemcpy(out_second, dS, 3 * nn * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_nvalid, dN, nn * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  return rc;
}

// ---------------------------------------------------------------------------
// contact-based dexterous-hand sampler (csrc/mgs_contact.hip)

int mgs_kin_desc_size(void) { return (int)sizeof(mgs_kin_desc); }

int mgs_contact_fps(int device, const double* points, int n, int k, int32_t* out_idx, double* kernel_ms) {
  if (n < 0 || k < 0 || (k > 0 && n == 0) || k > n) return fail(MGS_EINVAL, "mgs_contact_fps: need 0 <= k <= n%s");
  if (k == 0) return MGS_OK;
  if (!points || !out_idx) return fail(MGS_EINVAL, "mgs_contact_fps: null argument%s");
  HIPCHK(hipSetDevice(device));
  DevBufs b;
  double* dX = b.get<double>(3 * (size_t)n);
  double* dD = b.get<double>((size_t)n);
  int32_t* dO = b.get<int32_t>((size_t)k);
  if (!b.ok) return fail(MGS_ENOMEM, "device allocation failed%s");
  HIPCHK(hipMemcpy(dX, points, 3 * (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  EvTimer t;
  hipLaunchKernelGGL(mgs_fps_kernel, dim3(1), dim3(MGS_FPS_THREADS), 0, nullptr, dX, n, k, dD, dO);
  int rc = t.finish(kernel_ms);
  if (rc == MGS_OK) HIPCHK(hipMemcpy(out_idx, dO, (size_t)k * sizeof(int32_t), hipMemcpyDeviceToHost));
  return rc;
}

int mgs_contact_seeds(int device, const double* seeds, int k, double radius, uint64_t rng_seed, int ntip,
                      int32_t* out_nn, int32_t* out_sel, double* kernel_ms) {
  if (k < 0 || ntip < 1 || ntip > MGS_KIN_MAXTIP) return fail(MGS_EINVAL, "mgs_contact_seeds: bad size%s");
  if (k == 0) return MGS_OK;
  if (!seeds || !out_nn || !out_sel) return fail(MGS_EINVAL, "mgs_contact_seeds: null argument%s");
  HIPCHK(hipSetDevice(device));
  DevBufs b;
  double* dS = b.get<double>(3 * (size_t)k);
  int32_t* dN = b.get<int32_t>((size_t)k);
  int32_t* dL = b.get<int32_t>((size_t)k * ntip);
  if (!b.ok) return fail(MGS_ENOMEM, "device allocation failed%s");
  HIPCHK(hipMemcpy(dS, seeds, 3 * (size_t)k * sizeof(double), hipMemcpyHostToDevice));
  EvTimer t;
  hipLaunchKernelGGL(mgs_seeds_kernel, dim3((k + MGS_SEED_TILE - 1) / MGS_SEED_TILE), dim3(MGS_SEED_TILE), 0,
                     nullptr, dS, k, radius, rng_seed, ntip, dN, dL);
  int rc = t.finish(kernel_ms);
  if (rc == MGS_OK) {
    HIPCHK(hipMemcpy(out_nn, dN, (size_t)k * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_sel, dL, (size_t)k * ntip * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  return rc;
}

int mgs_contact_optimize(int device, const mgs_kin_desc* kin, int n, const double* rot_init, const double* pos_init,
                         const double* targets, const double* normals, double* out_rot, double* out_pos,
                         double* out_joints, double* out_loss, double* kernel_ms) {
  if (!kin || n < 0) return fail(MGS_EINVAL, "mgs_contact_optimize: bad argument%s");
  if (kin->ndof < 1 || kin->ndof > MGS_KIN_MAXDOF || kin->ntip < 1 || kin->ntip > MGS_KIN_MAXTIP ||
      kin->nperm < 1 || kin->nperm > MGS_KIN_MAXPERM || kin->iters < 0)
    return fail(MGS_EINVAL, "mgs_contact_optimize: kinematic model out of range%s");
  for (int a = 0; a < kin->ntip; a++) {
    if (kin->chain_len[a] < 1 || kin->chain_len[a] > MGS_KIN_MAXCHAIN)
      return fail(MGS_EINVAL, "mgs_contact_optimize: chain length out of range%s");
    for (int s = 0; s < kin->chain_len[a]; s++)
      if (kin->chain[a][s] < 0 || kin->chain[a][s] >= kin->ndof)
        return fail(MGS_EINVAL, "mgs_contact_optimize: chain dof out of range%s");
  }
  for (int q = 0; q < kin->nperm; q++)
    for (int a = 0; a < kin->ntip; a++)
      if (kin->perm[q][a] < 0 || kin->perm[q][a] >= kin->ntip)
        return fail(MGS_EINVAL, "mgs_contact_optimize: permutation entry out of range%s");
  if (n == 0) return MGS_OK;
  if (!rot_init || !pos_init || !targets || !normals || !out_rot || !out_pos || !out_joints)
    return fail(MGS_EINVAL, "mgs_contact_optimize: null argument%s");
  HIPCHK(hipSetDevice(device));
  const size_t nt = (size_t)kin->ntip, nd = (size_t)kin->ndof, nn = (size_t)n;
  DevBufs b;
  mgs_kin_desc* dK = b.get<mgs_kin_desc>(1);
  double* dR = b.get<double>(9 * nn);
  double* dP = b.get<double>(3 * nn);
  double* dT = b.get<double>(3 * nt * nn);
  double* dN = b.get<double>(3 * nt * nn);
  double* oR = b.get<double>(9 * nn);
  double* oP = b.get<double>(3 * nn);
  double* oJ = b.get<double>(nd * nn);
  double* oL = b.get<double>(nn);
  if (!b.ok) return fail(MGS_ENOMEM, "device allocation failed%s");
  HIPCHK(hipMemcpy(dK, kin, sizeof(mgs_kin_desc), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dR, rot_init, 9 * nn * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dP, pos_init, 3 * nn * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dT, targets, 3 * nt * nn * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dN, normals, 3 * nt * nn * sizeof(double), hipMemcpyHostToDevice));
  EvTimer t;
  hipLaunchKernelGGL(mgs_contact_opt_kernel, dim3((n + 63) / 64), dim3(64), 0, nullptr, dK, n, dR, dP, dT, dN,
                     oR, oP, oJ, oL);
  int rc = t.finish(kernel_ms);
  if (rc == MGS_OK) {
    HIPCHK(hipMemcpy(out_rot, oR, 9 * nn * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_pos, oP, 3 * nn * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_joints, oJ, nd * nn * sizeof(double), hipMemcpyDeviceToHost));
    if (out_loss) HIPCHK(hipMemcpy(out_loss, oL, nn * sizeof(double), hipMemcpyDeviceToHost));
  }
  return rc;
}

// ---------------------------------------------------------------------------
// scene scan (csrc/mgs_scan.hip)
}  // extern "C"
namespace {
// every index the scan kernel follows, checked on the host: "" or what is wrong
const char* scan_scene_error(const mgs_scan_scene* s) {
  if (s->ndraw < 0 || s->nmesh < 0 || s->nnode < 0 || s->ntri < 0) return "negative count";
  if (s->ndraw > 0 && (!s->draw_type || !s->draw_id || !s->draw_mesh || !s->draw_pos || !s->draw_rot || !s->draw_size))
    return "null drawable array";
  if (s->nmesh > 0 && (!s->mesh_node0 || !s->mesh_tri0)) return "null mesh range array";
  if (s->nnode > 0 && (!s->node_box || !s->node_skip || !s->node_first || !s->node_count)) return "null node array";
  if (s->ntri > 0 && (!s->tri || !s->tri_face)) return "null triangle array";
  for (int m = 0; m < s->nmesh; m++) {
    const int n0 = s->mesh_node0[m], n1 = s->mesh_node0[m + 1], t0 = s->mesh_tri0[m], t1 = s->mesh_tri0[m + 1];
    if (n0 < 0 || n1 < n0 || n1 > s->nnode || t0 < 0 || t1 < t0 || t1 > s->ntri) return "mesh range out of bounds";
    for (int i = 0; i < n1 - n0; i++) {
      const int g = n0 + i, cnt = s->node_count[g], first = s->node_first[g], skip = s->node_skip[g];
      if (skip <= i || skip > n1 - n0) return "skip index not forward or out of range";
      if (cnt < 0) return "negative leaf count";
      if (cnt > 0 && (first < 0 || first > t1 - t0 - cnt)) return "leaf triangles out of range";
      if (cnt == 0 && i + 1 >= n1 - n0) return "inner node without a child";
    }
  }
  for (int d = 0; d < s->ndraw; d++) {
    const int t = s->draw_type[d];
    if (t != MGS_SCAN_BOX && t != MGS_SCAN_SPHERE && t != MGS_SCAN_MESH && t != MGS_SCAN_CAPSULE &&
        t != MGS_SCAN_CYLINDER)
      return "unknown drawable type";
    if (t == MGS_SCAN_MESH && (s->draw_mesh[d] < 0 || s->draw_mesh[d] >= s->nmesh)) return "mesh index out of range";
    if (t == MGS_SCAN_CAPSULE || t == MGS_SCAN_CYLINDER) {
      const double r = s->draw_size[3 * (size_t)d], h = s->draw_size[3 * (size_t)d + 1];
      // written so that a NaN fails: radius finite and > 0, half-length finite and >= 0
      if (!(r > 0.0 && is_finite(r) && h >= 0.0 && is_finite(h))) {
        static thread_local char msg[96];
        snprintf(msg, sizeof(msg), "drawable %d: a %s needs a finite radius > 0 and a finite half-length >= 0", d,
                 t == MGS_SCAN_CAPSULE ? "capsule" : "cylinder");
        return msg;
      }
    }
  }
  return "";
}
// a checked scene's arrays on the device
ScanDev scan_upload_scene(DevBufs& b, const mgs_scan_scene* scene) {
  const size_t nd = (size_t)scene->ndraw, nm = (size_t)scene->nmesh, nn = (size_t)scene->nnode, nt = (size_t)scene->ntri;
  ScanDev S;
  S.ndraw = scene->ndraw;
  S.dtype = upload(b, scene->draw_type, nd);
  S.did = upload(b, scene->draw_id, nd);
  S.dmesh = upload(b, scene->draw_mesh, nd);
  S.dpos = upload(b, scene->draw_pos, 3 * nd);
  S.drot = upload(b, scene->draw_rot, 9 * nd);
  S.dsize = upload(b, scene->draw_size, 3 * nd);
  S.mnode0 = upload(b, scene->mesh_node0, nm ? nm + 1 : 0);
  S.mtri0 = upload(b, scene->mesh_tri0, nm ? nm + 1 : 0);
  S.nbox = upload(b, scene->node_box, 6 * nn);
  S.nskip = upload(b, scene->node_skip, nn);
  S.nfirst = upload(b, scene->node_first, nn);
  S.ncount = upload(b, scene->node_count, nn);
  S.tri = upload(b, scene->tri, 9 * nt);
  S.face = upload(b, scene->tri_face, nt);
  return S;
}
// the view arguments of the entry named `entry` (a render's views are its
// grid's z: at most 65535); *npix = the pixels of all views
int check_views(const char* entry, int nview, int width, int height, double fx, double fy, bool render, size_t* npix) {
  if (nview < 0 || width < 0 || height < 0) return fail(MGS_EINVAL, "%s: negative size", entry);
  if (render && nview > 65535) return fail(MGS_EINVAL, "%s: at most 65535 views per call", entry);
  if (!(fx > 0.0) || !(fy > 0.0)) return fail(MGS_EINVAL, "%s: focal lengths must be positive", entry);
  *npix = (size_t)nview * (size_t)width * (size_t)height;
  if (*npix > (size_t)1 << 30) return fail(MGS_EINVAL, "%s: more than 2^30 pixels", entry);
  return MGS_OK;
}
// the region mgs_scan_points keeps when the caller names none (the reference's)
const double ref_region[6] = {-0.25, -0.25, -0.01, 0.25, 0.25, 1.0};
// depth, segmentation, face id and triangle-test count of every pixel, on the null stream
void launch_scan_render(const ScanDev& S, const double* dP, const double* dR, int nview, int width, int height,
                        double fx, double fy, double cx, double cy, double* oD, int32_t* oS, int32_t* oT, int32_t* oN) {
  hipLaunchKernelGGL(mgs_scan_kernel,
                     dim3((width + MGS_SCAN_TILE - 1) / MGS_SCAN_TILE, (height + MGS_SCAN_TILE - 1) / MGS_SCAN_TILE, nview),
                     dim3(MGS_SCAN_TILE * MGS_SCAN_TILE), 0, nullptr, S, dP, dR, width, height, fx, fy, cx, cy, oD, oS,
                     oT, oN);
}
}  // namespace
extern "C" {

int mgs_scan_render(int device, const mgs_scan_scene* scene, int nview, const double* cam_pos,
                    const double* cam_rot, int width, int height, double fx, double fy, double cx, double cy,
                    double* out_depth, int32_t* out_seg, int32_t* out_tri, int32_t* out_ntest, double* kernel_ms) {
  if (!scene) return fail(MGS_EINVAL, "mgs_scan_render: null scene%s");
  size_t n = 0;
  if (int rc = check_views("mgs_scan_render", nview, width, height, fx, fy, true, &n)) return rc;
  const char* bad = scan_scene_error(scene);
  if (bad[0]) return fail(MGS_EINVAL, "mgs_scan_render: scene: %s", bad);
  if (n == 0) return MGS_OK;
  if (!cam_pos || !cam_rot || !out_depth || !out_seg || !out_tri)
    return fail(MGS_EINVAL, "mgs_scan_render: null argument%s");
  HIPCHK(hipSetDevice(device));
  DevBufs b;
  ScanDev S = scan_upload_scene(b, scene);
  double* dP = upload(b, cam_pos, 3 * (size_t)nview);
  double* dR = upload(b, cam_rot, 9 * (size_t)nview);
  double* oD = b.get<double>(n);
  int32_t* oS = b.get<int32_t>(n);
  int32_t* oT = b.get<int32_t>(n);
  int32_t* oN = b.get<int32_t>(n);
  if (!b.ok) return fail(MGS_ENOMEM, "device allocation or upload failed%s");
  EvTimer t;
  launch_scan_render(S, dP, dR, nview, width, height, fx, fy, cx, cy, oD, oS, oT, oN);
  int rc = t.finish(kernel_ms);
  if (rc == MGS_OK) {
    HIPCHK(hipMemcpy(out_depth, oD, n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_seg, oS, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_tri, oT, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (out_ntest) HIPCHK(hipMemcpy(out_ntest, oN, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  return rc;
}

int mgs_scan_points(int device, int nview, int width, int height, const double* depth, const int32_t* seg,
                    const double* extrinsics, double fx, double fy, double cx, double cy, int erode_iters,
                    const double* region, double* out_points, uint8_t* out_keep, double* kernel_ms) {
  size_t n = 0;
  if (int rc = check_views("mgs_scan_points", nview, width, height, fx, fy, false, &n)) return rc;
  if (erode_iters < 0 || erode_iters > 64) return fail(MGS_EINVAL, "mgs_scan_points: erode_iters must be 0 .. 64%s");
  if (n == 0) return MGS_OK;
  if (!depth || !seg || !extrinsics || !out_points || !out_keep)
    return fail(MGS_EINVAL, "mgs_scan_points: null argument%s");
  const double* rg = region ? region : ref_region;
  HIPCHK(hipSetDevice(device));
  DevBufs b;
  double* dD = upload(b, depth, n);
  int32_t* dS = upload(b, seg, n);
  double* dE = upload(b, extrinsics, 16 * (size_t)nview);
  double* oP = b.get<double>(3 * n);
  uint8_t* oK = b.get<uint8_t>(n);
  if (!b.ok) return fail(MGS_ENOMEM, "device allocation or upload failed%s");
  EvTimer t;
  hipLaunchKernelGGL(mgs_scan_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, nview, width,
                     height, dD, dS, dE, fx, fy, cx, cy, erode_iters, rg[0], rg[1], rg[2], rg[3], rg[4], rg[5], oP, oK);
  int rc = t.finish(kernel_ms);
  if (rc == MGS_OK) {
    HIPCHK(hipMemcpy(out_points, oP, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_keep, oK, n * sizeof(uint8_t), hipMemcpyDeviceToHost));
  }
  return rc;
}

// ---------------------------------------------------------------------------
// scene cloud (csrc/mgs_cloud.hip)
}  // extern "C"
namespace {
struct CloudVox {      // what the voxel stage leaves on the device (buffers owned by the caller's DevBufs)
  uint32_t npts = 0, nvox = 0;
  int64_t ncell = 0;
  double* vpts = nullptr;
  float* vfeat = nullptr;
  int32_t* vcnt = nullptr;
};

size_t cloud_blocks(size_t n) { return (n + MGS_CLOUD_CHUNK - 1) / MGS_CLOUD_CHUNK; }

// min / max / non-finite flag / kept count of x (n * 3) under keep (or NULL),
// and the exclusive scan of the per-block kept counts in *sums
int cloud_bounds(DevBufs& b, const double* dX, const uint8_t* dK, size_t n, cloud_u64** sums, CloudHdr* h) {
  const size_t nb = cloud_blocks(n);
  *sums = b.get<cloud_u64>(nb);
  double* blo = b.get<double>(3 * nb);
  double* bhi = b.get<double>(3 * nb);
  int32_t* bbad = b.get<int32_t>(nb);
  CloudHdr* dH = b.get<CloudHdr>(1);
  if (!b.ok) return fail(MGS_ENOMEM, "device allocation failed%s");
  hipLaunchKernelGGL(cloud_flag_kernel, dim3((unsigned)nb), dim3(MGS_CLOUD_BLOCK), 0, nullptr, dX, dK, n, *sums, blo,
                     bhi, bbad);
  hipLaunchKernelGGL(cloud_scan_sums_kernel, dim3(1), dim3(MGS_CLOUD_BLOCK), 0, nullptr, *sums, nb, blo, bhi, bbad, dH);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(h, dH, sizeof(CloudHdr), hipMemcpyDeviceToHost));
  return MGS_OK;
}

// counted grid (ncell) and the points' cells (npts) -> *start (occupied + 1:
// first slot of every occupied cell in ascending cell, then npts), *slot_idx
// (npts: point per slot, unordered inside a cell), *nocc.  cap >= 0: more
// occupied cells than cap is MGS_ECAPACITY with *nocc set.  *start and
// *slot_idx come from `keep`, what only this step needs from `b` (the two may
// be one; a batch keeps the first and releases the second scene by scene).
int cloud_slots(DevBufs& b, DevBufs& keep, uint32_t* grid, size_t ncell, const uint32_t* pcell, uint32_t npts,
                int64_t cap, uint32_t** start, uint32_t** slot_idx, uint32_t* nocc) {
  const size_t nb = cloud_blocks(ncell);
  cloud_u64* sums = b.get<cloud_u64>(nb);
  CloudHdr* dH = b.get<CloudHdr>(1);
  if (!b.ok) return fail(MGS_ENOMEM, "device allocation failed%s");
  hipLaunchKernelGGL(cloud_cell_sums_kernel, dim3((unsigned)nb), dim3(MGS_CLOUD_BLOCK), 0, nullptr, grid, ncell, sums);
  hipLaunchKernelGGL(cloud_scan_sums_kernel, dim3(1), dim3(MGS_CLOUD_BLOCK), 0, nullptr, sums, nb,
                     (const double*)nullptr, (const double*)nullptr, (const int32_t*)nullptr, dH);
  HIPCHK(hipGetLastError());
  CloudHdr h;
  HIPCHK(hipMemcpy(&h, dH, sizeof(cloud_u64), hipMemcpyDeviceToHost));
  *nocc = (uint32_t)(h.total >> 32);
  if ((uint32_t)h.total != npts || *nocc > npts) return fail(MGS_EHIP, "cloud grid: the cell counts do not add up%s");
  if (cap >= 0 && (int64_t)*nocc > cap) return MGS_ECAPACITY;
  *start = keep.get<uint32_t>((size_t)*nocc + 1);
  *slot_idx = keep.get<uint32_t>(npts);
  if (!keep.ok) return fail(MGS_ENOMEM, "device allocation failed%s");
  hipLaunchKernelGGL(cloud_cell_offsets_kernel, dim3((unsigned)nb), dim3(MGS_CLOUD_BLOCK), 0, nullptr, grid, ncell, sums,
                     *start, *nocc, npts);
  hipLaunchKernelGGL(cloud_scatter_kernel, dim3((npts + MGS_CLOUD_BLOCK - 1) / MGS_CLOUD_BLOCK), dim3(MGS_CLOUD_BLOCK),
                     0, nullptr, pcell, npts, grid, *slot_idx);
  HIPCHK(hipGetLastError());
  return MGS_OK;
}

// the voxel stage on device arrays: dX (n * 3), dK (n or NULL), features dF
// (n * nfeat) or, with dSeg, the rows dCol[dSeg] (nfeat 3).  `mid` (or NULL)
// is recorded behind the compaction.  cap as cloud_slots.  The voxels V leaves
// come from `keep`, everything else from `b` (as cloud_slots).
int cloud_voxels_dev(DevBufs& b, DevBufs& keep, const double* dX, const uint8_t* dK, size_t n, const float* dF, int nfeat,
                     const int32_t* dSeg, const float* dCol, int ncolor, double voxel_size, int64_t cap, CloudVox* V,
                     hipEvent_t mid) {
  *V = CloudVox();
  int rc = MGS_OK;
  cloud_u64* sums = nullptr;
  CloudHdr h;
  if (n > 0) rc = cloud_bounds(b, dX, dK, n, &sums, &h);
  if (rc != MGS_OK || n == 0 || h.total == 0) {
    if (mid) hipEventRecord(mid, nullptr);
    return rc;
  }
  if (h.bad) return fail(MGS_EINVAL, "cloud voxels: a kept point is not finite%s");
  CloudGrid G;
  int64_t ncell = 1;
  for (int k = 0; k < 3; k++) {
    const double f = cloud_floor_divide(h.hi[k] - h.lo[k], voxel_size);
    if (!(f < 4.0e18)) return fail(MGS_EINVAL, "cloud voxels: the grid's raveled index overflows int64%s");
    G.lo[k] = h.lo[k];
    G.dim[k] = (int64_t)f + 1;
    if (__builtin_mul_overflow(ncell, G.dim[k], &ncell))
      return fail(MGS_EINVAL, "cloud voxels: the grid's raveled index overflows int64%s");
  }
  G.side = voxel_size;
  V->ncell = ncell;
  if (ncell > (int64_t)MGS_CLOUD_MAX_CELLS) {
    V->nvox = 0xffffffffu;
    return fail(MGS_ECAPACITY, "cloud voxels: the grid has more than MGS_CLOUD_MAX_CELLS cells%s");
  }
  const uint32_t m = (uint32_t)h.total;
  V->npts = m;
  double* cpts = b.get<double>(3 * (size_t)m);
  float* cfeat = b.get<float>((size_t)nfeat * m);
  uint32_t* pcell = b.get<uint32_t>(m);
  uint32_t* grid = b.get<uint32_t>((size_t)ncell);
  if (!b.ok) return fail(MGS_ENOMEM, "device allocation failed%s");
  HIPCHK(hipMemsetAsync(grid, 0, (size_t)ncell * sizeof(uint32_t), nullptr));
  hipLaunchKernelGGL(cloud_compact_kernel, dim3((unsigned)cloud_blocks(n)), dim3(MGS_CLOUD_BLOCK), 0, nullptr, dX, dK, n,
                     sums, dF, nfeat, dSeg, dCol, ncolor, G, cpts, cfeat, pcell, grid);
  if (mid) hipEventRecord(mid, nullptr);
  uint32_t *start = nullptr, *slot_idx = nullptr;
  rc = cloud_slots(b, b, grid, (size_t)ncell, pcell, m, cap, &start, &slot_idx, &V->nvox);
  if (rc != MGS_OK) return rc == MGS_ECAPACITY ? fail(rc, "cloud voxels: more voxels than the outputs hold%s") : rc;
  V->vpts = keep.get<double>(3 * (size_t)V->nvox);
  V->vfeat = keep.get<float>((size_t)nfeat * V->nvox);
  V->vcnt = keep.get<int32_t>(V->nvox);
  if (!keep.ok) return fail(MGS_ENOMEM, "device allocation failed%s");
  hipLaunchKernelGGL(cloud_voxel_kernel, dim3((V->nvox + MGS_CLOUD_BLOCK - 1) / MGS_CLOUD_BLOCK), dim3(MGS_CLOUD_BLOCK),
                     0, nullptr, start, V->nvox, slot_idx, cpts, cfeat, nfeat, V->vpts, V->vfeat, V->vcnt);
  HIPCHK(hipGetLastError());
  return MGS_OK;
}

// the pick's set-up on device arrays: dX (n * 3, finite), 1 <= k <= n; dOut (k),
// dEv (1).  *J = the arguments of the pick; the arrays they name come from
// `keep` and live until the pick has run, the set-up's own from `b`.
int cloud_fps_setup(DevBufs& b, DevBufs& keep, const double* dX, int n, int k, double bucket_size, int32_t* dOut,
                    cloud_u64* dEv, CloudFpsJob* J) {
  cloud_u64* sums = nullptr;
  CloudHdr h;
  int rc = cloud_bounds(b, dX, nullptr, (size_t)n, &sums, &h);
  if (rc != MGS_OK) return rc;
  if (h.bad) return fail(MGS_EINVAL, "cloud pick: a point is not finite%s");
  double ext[3];
  for (int a = 0; a < 3; a++) {
    ext[a] = h.hi[a] - h.lo[a];
    if (!is_finite(ext[a])) return fail(MGS_EINVAL, "cloud pick: the points' extent is not finite%s");
  }
  CloudGrid G;
  double side = bucket_size, d[3];
  for (;;) {
    for (int a = 0; a < 3; a++) d[a] = floor(ext[a] / side) + 1.0;
    if (d[0] * d[1] * d[2] <= (double)MGS_CLOUD_FPS_MAX_CELLS) break;
    side = side * 2.0;
  }
  for (int a = 0; a < 3; a++) { G.lo[a] = h.lo[a]; G.dim[a] = (int64_t)d[a]; }
  G.side = side;
  const size_t ncell = (size_t)(G.dim[0] * G.dim[1] * G.dim[2]);
  uint32_t* pcell = b.get<uint32_t>((size_t)n);
  uint32_t* grid = b.get<uint32_t>(ncell);
  if (!b.ok) return fail(MGS_ENOMEM, "device allocation failed%s");
  HIPCHK(hipMemsetAsync(grid, 0, ncell * sizeof(uint32_t), nullptr));
  const unsigned pb = ((unsigned)n + MGS_CLOUD_BLOCK - 1) / MGS_CLOUD_BLOCK;
  hipLaunchKernelGGL(cloud_fps_cell_kernel, dim3(pb), dim3(MGS_CLOUD_BLOCK), 0, nullptr, dX, (uint32_t)n, G, pcell, grid);
  uint32_t *start = nullptr, *slot_idx = nullptr, nbkt = 0;
  rc = cloud_slots(b, keep, grid, ncell, pcell, (uint32_t)n, -1, &start, &slot_idx, &nbkt);
  if (rc != MGS_OK) return rc;
  double* bx = keep.get<double>(3 * (size_t)n);
  double* bdist = keep.get<double>((size_t)n);
  double* bbox = keep.get<double>(6 * (size_t)nbkt);
  double* bmax = keep.get<double>(nbkt);
  int32_t* bidx = keep.get<int32_t>(nbkt);
  if (!keep.ok) return fail(MGS_ENOMEM, "device allocation failed%s");
  hipLaunchKernelGGL(cloud_fps_gather_kernel, dim3(pb), dim3(MGS_CLOUD_BLOCK), 0, nullptr, dX, (uint32_t)n, slot_idx, bx,
                     bdist);
  hipLaunchKernelGGL(cloud_fps_box_kernel, dim3((nbkt + MGS_CLOUD_BLOCK - 1) / MGS_CLOUD_BLOCK), dim3(MGS_CLOUD_BLOCK), 0,
                     nullptr, start, nbkt, slot_idx, bx, bbox, bmax, bidx);
  HIPCHK(hipGetLastError());
  *J = CloudFpsJob{dX, bx, slot_idx, bdist, start, bbox, bmax, bidx, dOut, dEv, (int32_t)nbkt, (int32_t)k};
  return MGS_OK;
}

// one cloud's pick: its set-up and the single-cloud kernel
int cloud_fps_dev(DevBufs& b, const double* dX, int n, int k, double bucket_size, int32_t* dOut, cloud_u64* dEv) {
  CloudFpsJob J;
  int rc = cloud_fps_setup(b, b, dX, n, k, bucket_size, dOut, dEv, &J);
  if (rc != MGS_OK) return rc;
  hipLaunchKernelGGL(mgs_cloud_fps_kernel, dim3(1), dim3(MGS_CLOUD_FPS_THREADS), 0, nullptr, J.x, J.bx, J.borig, J.bdist,
                     J.start, J.bbox, J.bmax, J.bidx, (int)J.nb, (int)J.k, J.out, J.nevals);
  HIPCHK(hipGetLastError());
  return MGS_OK;
}

// heaviest first: descending n * k, equal work by ascending index
void cloud_fps_order(int ncloud, const int64_t* n, const int32_t* k, int32_t* order) {
  for (int c = 0; c < ncloud; c++) order[c] = c;
  std::stable_sort(order, order + ncloud, [&](int32_t a, int32_t b) { return n[a] * (int64_t)k[a] > n[b] * (int64_t)k[b]; });
}

// the picks of jobs (n[j] = the points of job j) in one launch, heaviest first; *ms (or NULL) = its time
int cloud_fps_launch_batch(DevBufs& b, const std::vector<CloudFpsJob>& jobs, const std::vector<int64_t>& n, double* ms) {
  if (ms) *ms = 0.0;
  const int nj = (int)jobs.size();
  if (nj == 0) return MGS_OK;
  std::vector<int32_t> k(nj), order(nj);
  for (int j = 0; j < nj; j++) k[j] = jobs[j].k;
  cloud_fps_order(nj, n.data(), k.data(), order.data());
  std::vector<CloudFpsJob> table(nj);
  for (int j = 0; j < nj; j++) table[j] = jobs[order[j]];
  CloudFpsJob* dJ = upload(b, table.data(), (size_t)nj);
  if (!b.ok) return fail(MGS_ENOMEM, "device allocation or upload failed%s");
  EvTimer t;
  hipLaunchKernelGGL(mgs_cloud_fps_batch_kernel, dim3((unsigned)nj), dim3(MGS_CLOUD_FPS_THREADS), 0, nullptr, dJ);
  return t.finish(ms);
}

// the current error text behind "<entry>: <what> <index>: "
int fail_at(int rc, const char* entry, const char* what, int index) {
  const std::string inner = g_err;
  char head[128];
  snprintf(head, sizeof(head), "%s: %s %d: ", entry, what, index);
  g_err = head + inner;
  return rc;
}

bool cloud_size_ok(double v) { return v > 0.0 && is_finite(v); }

// the argument rules of mgs_scan_fps (one cloud of mgs_scan_fps_batch)
int scan_fps_check(const double* points, int64_t n, int64_t k, double bucket_size, const int32_t* out_idx) {
  if (n < 0 || k < 0 || (k > 0 && n == 0) || k > n) return fail(MGS_EINVAL, "mgs_scan_fps: need 0 <= k <= n%s");
  if (n > 0x7fffffff) return fail(MGS_EINVAL, "mgs_scan_fps: more than 2^31 - 1 points%s");
  if (!cloud_size_ok(bucket_size)) return fail(MGS_EINVAL, "mgs_scan_fps: bucket_size must be positive and finite%s");
  if (k > 0 && (!points || !out_idx)) return fail(MGS_EINVAL, "mgs_scan_fps: null argument%s");
  if (k > 0)
    for (size_t j = 0; j < 3 * (size_t)n; j++)
      if (!is_finite(points[j])) return fail(MGS_EINVAL, "mgs_scan_fps: a point is not finite%s");
  return MGS_OK;
}

// the argument rules of mgs_scan_cloud: what every scene of a batch shares ...
int scan_cloud_check_views(const char* entry, int nview, const double* cam_pos, const double* cam_rot, int width,
                           int height, double fx, double fy, const double* extrinsics, double pfx, double pfy,
                           int erode_iters, double voxel_size, size_t* npix) {
  if (int rc = check_views(entry, nview, width, height, fx, fy, true, npix)) return rc;
  if (!(pfx > 0.0) || !(pfy > 0.0)) return fail(MGS_EINVAL, "%s: focal lengths must be positive", entry);
  if (erode_iters < 0 || erode_iters > 64) return fail(MGS_EINVAL, "%s: erode_iters must be 0 .. 64", entry);
  if (!cloud_size_ok(voxel_size)) return fail(MGS_EINVAL, "%s: voxel_size must be positive and finite", entry);
  if (*npix > 0 && (!cam_pos || !cam_rot || !extrinsics)) return fail(MGS_EINVAL, "%s: null argument", entry);
  return MGS_OK;
}
// ... and one scene's own
int scan_cloud_check_scene(const mgs_scan_scene* scene, const float* colors, int ncolor, int num_points,
                           const float* out_points, const float* out_colors) {
  if (!scene) return fail(MGS_EINVAL, "mgs_scan_cloud: null scene%s");
  if (num_points < 0 || ncolor < 0) return fail(MGS_EINVAL, "mgs_scan_cloud: negative size%s");
  const char* bad = scan_scene_error(scene);
  if (bad[0]) return fail(MGS_EINVAL, "mgs_scan_cloud: scene: %s", bad);
  for (int d = 0; d < scene->ndraw; d++)
    if (scene->draw_id[d] < 0 || scene->draw_id[d] >= ncolor)
      return fail(MGS_EINVAL, "mgs_scan_cloud: a draw_id has no row of colors%s");
  if ((ncolor > 0 && !colors) || (num_points > 0 && (!out_points || !out_colors)))
    return fail(MGS_EINVAL, "mgs_scan_cloud: null argument%s");
  return MGS_OK;
}

struct CloudEvents {
  hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  CloudEvents() { for (auto& x : e) hipEventCreate(&x); }
  ~CloudEvents() { for (auto& x : e) hipEventDestroy(x); }
};

// what mgs_scan_cloud_batch shares between its scenes, on the device: the
// cameras and the images (every scene renders into the same ones)
struct CloudBatchViews {
  size_t n = 0;
  int nview = 0, width = 0, height = 0, erode_iters = 0;
  double fx = 0, fy = 0, cx = 0, cy = 0, pfx = 0, pfy = 0, pcx = 0, pcy = 0, voxel_size = 0;
  const double* rg = nullptr;
  double *dCP = nullptr, *dCR = nullptr, *dE = nullptr, *dD = nullptr, *dD32 = nullptr, *dP = nullptr;
  int32_t *dS = nullptr, *dT = nullptr, *dN = nullptr;
  uint8_t* dK = nullptr;
};
// what one scene of a batch leaves on the device until the batched pick
struct CloudBatchScene {
  CloudVox V;
  int m = 0;                      // rows it returns
  float *oP = nullptr, *oC = nullptr;
  int32_t* dIdx = nullptr;        // the pick's indices (NULL: every voxel in voxel order)
  double ms[3] = {0.0, 0.0, 0.0};
};
// render, points, compaction and voxels of one scene, and its pick's set-up
// (*picked, *J).  The scene's own arrays (its drawables, the compacted points,
// the dense grid, the set-up's grid) live in a DevBufs of this call, released
// on return; what the pick and the output need comes from `keep`.
int cloud_batch_scene(DevBufs& keep, const CloudBatchViews& v, const mgs_scan_cloud_job& job, cloud_u64* dEv,
                      CloudBatchScene* out, bool* picked, CloudFpsJob* J) {
  DevBufs s;
  ScanDev S = scan_upload_scene(s, job.scene);
  float* dCol = upload(s, job.colors, 3 * (size_t)job.ncolor);
  if (!s.ok) return fail(MGS_ENOMEM, "device allocation or upload failed%s");
  CloudEvents ev;
  hipEventRecord(ev.e[0], nullptr);
  launch_scan_render(S, v.dCP, v.dCR, v.nview, v.width, v.height, v.fx, v.fy, v.cx, v.cy, v.dD, v.dS, v.dT, v.dN);
  hipEventRecord(ev.e[1], nullptr);
  hipLaunchKernelGGL(cloud_round_f32_kernel, dim3((unsigned)((v.n + MGS_CLOUD_BLOCK - 1) / MGS_CLOUD_BLOCK)),
                     dim3(MGS_CLOUD_BLOCK), 0, nullptr, v.dD, v.n, v.dD32);
  hipLaunchKernelGGL(mgs_scan_points_kernel, dim3((unsigned)((v.n + 255) / 256)), dim3(256), 0, nullptr, v.nview, v.width,
                     v.height, v.dD32, v.dS, v.dE, v.pfx, v.pfy, v.pcx, v.pcy, v.erode_iters, v.rg[0], v.rg[1], v.rg[2],
                     v.rg[3], v.rg[4], v.rg[5], v.dP, v.dK);
  HIPCHK(hipGetLastError());
  int rc = cloud_voxels_dev(s, keep, v.dP, v.dK, v.n, nullptr, 3, v.dS, dCol, job.ncolor, v.voxel_size, -1, &out->V,
                            ev.e[2]);
  if (rc != MGS_OK) return rc;
  hipEventRecord(ev.e[3], nullptr);
  const int nvox = (int)out->V.nvox;
  out->m = nvox >= job.num_points ? job.num_points : nvox;
  *picked = false;
  if (out->m > 0) {
    out->oP = keep.get<float>(3 * (size_t)out->m);
    out->oC = keep.get<float>(3 * (size_t)out->m);
    if (nvox >= job.num_points) {
      double* dX = keep.get<double>(3 * (size_t)nvox);
      out->dIdx = keep.get<int32_t>((size_t)out->m);
      if (!keep.ok) return fail(MGS_ENOMEM, "device allocation failed%s");
      hipLaunchKernelGGL(cloud_round_f32_kernel, dim3((3 * (unsigned)nvox + MGS_CLOUD_BLOCK - 1) / MGS_CLOUD_BLOCK),
                         dim3(MGS_CLOUD_BLOCK), 0, nullptr, out->V.vpts, 3 * (size_t)nvox, dX);
      rc = cloud_fps_setup(s, keep, dX, nvox, out->m, 8.0 * v.voxel_size, out->dIdx, dEv, J);
      if (rc != MGS_OK) return rc;
      *picked = true;
    }
    if (!keep.ok) return fail(MGS_ENOMEM, "device allocation failed%s");
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());      // the scene's own arrays go when this returns
  for (int i = 0; i < 3; i++) {
    float f = 0.f;
    hipEventElapsedTime(&f, ev.e[i], ev.e[i + 1]);
    out->ms[i] = f;
  }
  return MGS_OK;
}
}  // namespace
extern "C" {

int mgs_scan_voxels(int device, int n, const double* points, const uint8_t* keep, int nfeat, const float* features,
                    double voxel_size, int cap, double* out_points, float* out_features, int32_t* out_count,
                    int32_t* out_nvox, double* kernel_ms) {
  if (n < 0 || nfeat < 0 || cap < 0) return fail(MGS_EINVAL, "mgs_scan_voxels: negative size%s");
  if (n > (1 << 30)) return fail(MGS_EINVAL, "mgs_scan_voxels: more than 2^30 points%s");
  if (!cloud_size_ok(voxel_size)) return fail(MGS_EINVAL, "mgs_scan_voxels: voxel_size must be positive and finite%s");
  if (!out_nvox || (n > 0 && !points) || (n > 0 && nfeat > 0 && !features) ||
      (cap > 0 && (!out_points || (nfeat > 0 && !out_features))))
    return fail(MGS_EINVAL, "mgs_scan_voxels: null argument%s");
  for (size_t j = 0; j < (size_t)n; j++) {
    if (keep && !keep[j]) continue;
    for (int a = 0; a < 3; a++)
      if (!is_finite(points[3 * j + a])) return fail(MGS_EINVAL, "mgs_scan_voxels: a kept point is not finite%s");
  }
  if (n == 0) { *out_nvox = 0; return MGS_OK; }
  HIPCHK(hipSetDevice(device));
  DevBufs b;
  const size_t nn = (size_t)n;
  double* dX = upload(b, points, 3 * nn);
  uint8_t* dK = keep ? upload(b, keep, nn) : nullptr;
  float* dF = nfeat > 0 ? upload(b, features, (size_t)nfeat * nn) : nullptr;
  if (!b.ok) return fail(MGS_ENOMEM, "device allocation or upload failed%s");
  EvTimer t;
  CloudVox V;
  int rc = cloud_voxels_dev(b, b, dX, dK, nn, dF, nfeat, nullptr, nullptr, 0, voxel_size, cap, &V, nullptr);
  if (rc == MGS_ECAPACITY) { *out_nvox = (int32_t)V.nvox; return rc; }      // 0xffffffff = -1: the grid itself
  if (rc != MGS_OK) return rc;
  rc = t.finish(kernel_ms);
  if (rc != MGS_OK) return rc;
  const size_t nv = V.nvox;
  if (nv > 0) {
    HIPCHK(hipMemcpy(out_points, V.vpts, 3 * nv * sizeof(double), hipMemcpyDeviceToHost));
    if (nfeat > 0) HIPCHK(hipMemcpy(out_features, V.vfeat, (size_t)nfeat * nv * sizeof(float), hipMemcpyDeviceToHost));
    if (out_count) HIPCHK(hipMemcpy(out_count, V.vcnt, nv * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  *out_nvox = (int32_t)nv;
  return MGS_OK;
}

int mgs_scan_fps(int device, const double* points, int n, int k, double bucket_size, int32_t* out_idx,
                 int64_t* out_nevals, double* kernel_ms) {
  if (int rc = scan_fps_check(points, n, k, bucket_size, out_idx)) return rc;
  if (k == 0) {
    if (out_nevals) *out_nevals = 0;
    return MGS_OK;
  }
  HIPCHK(hipSetDevice(device));
  DevBufs b;
  double* dX = upload(b, points, 3 * (size_t)n);
  int32_t* dO = b.get<int32_t>((size_t)k);
  cloud_u64* dEv = b.get<cloud_u64>(1);
  if (!b.ok) return fail(MGS_ENOMEM, "device allocation or upload failed%s");
  EvTimer t;
  int rc = cloud_fps_dev(b, dX, n, k, bucket_size, dO, dEv);
  if (rc != MGS_OK) return rc;
  rc = t.finish(kernel_ms);
  if (rc != MGS_OK) return rc;
  cloud_u64 ev = 0;
  HIPCHK(hipMemcpy(&ev, dEv, sizeof(ev), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(out_idx, dO, (size_t)k * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (out_nevals) *out_nevals = (int64_t)ev;
  return MGS_OK;
}

int mgs_scan_cloud(int device, const mgs_scan_scene* scene, int nview, const double* cam_pos, const double* cam_rot,
                   int width, int height, double fx, double fy, double cx, double cy, const double* extrinsics,
                   double pfx, double pfy, double pcx, double pcy, int erode_iters, const double* region,
                   const float* colors, int ncolor, double voxel_size, int num_points, float* out_points,
                   float* out_colors, int32_t* out_n, int64_t* out_stats, double* stage_ms) {
  if (!scene) return fail(MGS_EINVAL, "mgs_scan_cloud: null scene%s");
  size_t n = 0;
  if (int rc = scan_cloud_check_views("mgs_scan_cloud", nview, cam_pos, cam_rot, width, height, fx, fy, extrinsics, pfx,
                                      pfy, erode_iters, voxel_size, &n))
    return rc;
  if (int rc = scan_cloud_check_scene(scene, colors, ncolor, num_points, out_points, out_colors)) return rc;
  if (!out_n) return fail(MGS_EINVAL, "mgs_scan_cloud: null argument%s");
  if (out_stats) for (int i = 0; i < 8; i++) out_stats[i] = 0;
  if (stage_ms) for (int i = 0; i < 4; i++) stage_ms[i] = 0.0;
  if (n == 0) { *out_n = 0; return MGS_OK; }
  const double* rg = region ? region : ref_region;
  HIPCHK(hipSetDevice(device));
  DevBufs b;
  ScanDev S = scan_upload_scene(b, scene);
  double* dCP = upload(b, cam_pos, 3 * (size_t)nview);
  double* dCR = upload(b, cam_rot, 9 * (size_t)nview);
  double* dE = upload(b, extrinsics, 16 * (size_t)nview);
  float* dCol = upload(b, colors, 3 * (size_t)ncolor);
  double* dD = b.get<double>(n);
  double* dD32 = b.get<double>(n);
  int32_t* dS = b.get<int32_t>(n);
  int32_t* dT = b.get<int32_t>(n);
  int32_t* dN = b.get<int32_t>(n);
  double* dP = b.get<double>(3 * n);
  uint8_t* dK = b.get<uint8_t>(n);
  if (!b.ok) return fail(MGS_ENOMEM, "device allocation or upload failed%s");
  CloudEvents ev;
  const unsigned pix_blocks = (unsigned)((n + MGS_CLOUD_BLOCK - 1) / MGS_CLOUD_BLOCK);
  hipEventRecord(ev.e[0], nullptr);
  launch_scan_render(S, dCP, dCR, nview, width, height, fx, fy, cx, cy, dD, dS, dT, dN);
  hipEventRecord(ev.e[1], nullptr);
  hipLaunchKernelGGL(cloud_round_f32_kernel, dim3(pix_blocks), dim3(MGS_CLOUD_BLOCK), 0, nullptr, dD, n, dD32);
  hipLaunchKernelGGL(mgs_scan_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, nview, width,
                     height, dD32, dS, dE, pfx, pfy, pcx, pcy, erode_iters, rg[0], rg[1], rg[2], rg[3], rg[4], rg[5], dP,
                     dK);
  HIPCHK(hipGetLastError());
  CloudVox V;
  int rc = cloud_voxels_dev(b, b, dP, dK, n, nullptr, 3, dS, dCol, ncolor, voxel_size, -1, &V, ev.e[2]);
  if (rc != MGS_OK) return rc;
  hipEventRecord(ev.e[3], nullptr);
  const int nvox = (int)V.nvox;
  const int m = nvox >= num_points ? num_points : nvox;
  cloud_u64 evals = 0;
  float *oP = nullptr, *oC = nullptr;
  if (m > 0) {
    oP = b.get<float>(3 * (size_t)m);
    oC = b.get<float>(3 * (size_t)m);
    int32_t* dIdx = nullptr;
    cloud_u64* dEv = nullptr;
    if (nvox >= num_points) {
      double* dX = b.get<double>(3 * (size_t)nvox);
      dIdx = b.get<int32_t>((size_t)m);
      dEv = b.get<cloud_u64>(1);
      if (!b.ok) return fail(MGS_ENOMEM, "device allocation failed%s");
      hipLaunchKernelGGL(cloud_round_f32_kernel, dim3((3 * (unsigned)nvox + MGS_CLOUD_BLOCK - 1) / MGS_CLOUD_BLOCK),
                         dim3(MGS_CLOUD_BLOCK), 0, nullptr, V.vpts, 3 * (size_t)nvox, dX);
      rc = cloud_fps_dev(b, dX, nvox, m, 8.0 * voxel_size, dIdx, dEv);
      if (rc != MGS_OK) return rc;
    }
    if (!b.ok) return fail(MGS_ENOMEM, "device allocation failed%s");
    hipLaunchKernelGGL(cloud_gather_kernel, dim3((m + MGS_CLOUD_BLOCK - 1) / MGS_CLOUD_BLOCK), dim3(MGS_CLOUD_BLOCK), 0,
                       nullptr, dIdx, m, V.vpts, V.vfeat, oP, oC);
    if (dEv) {
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpy(&evals, dEv, sizeof(evals), hipMemcpyDeviceToHost));
    }
  }
  hipEventRecord(ev.e[4], nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventSynchronize(ev.e[4]));
  if (m > 0) {
    HIPCHK(hipMemcpy(out_points, oP, 3 * (size_t)m * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_colors, oC, 3 * (size_t)m * sizeof(float), hipMemcpyDeviceToHost));
  }
  *out_n = m;
  if (stage_ms)
    for (int i = 0; i < 4; i++) {
      float f = 0.f;
      hipEventElapsedTime(&f, ev.e[i], ev.e[i + 1]);
      stage_ms[i] = f;
    }
  if (out_stats) {
    out_stats[0] = V.npts;
    out_stats[1] = nvox;
    out_stats[2] = (int64_t)evals;
    out_stats[3] = V.ncell;
    out_stats[4] = m;
    out_stats[5] = (int64_t)n;
  }
  return MGS_OK;
}

int mgs_scan_fps_order(int ncloud, const int64_t* n, const int32_t* k, int32_t* order) {
  if (ncloud < 0) return fail(MGS_EINVAL, "mgs_scan_fps_order: negative size%s");
  if (ncloud > 0 && (!n || !k || !order)) return fail(MGS_EINVAL, "mgs_scan_fps_order: null argument%s");
  cloud_fps_order(ncloud, n, k, order);
  return MGS_OK;
}

int mgs_scan_fps_batch(int device, int ncloud, const double* points, const int64_t* off, const int32_t* k,
                       double bucket_size, int32_t* out_idx, int64_t* out_nevals, double* kernel_ms) {
  const char* E = "mgs_scan_fps_batch";
  if (ncloud < 0) return fail(MGS_EINVAL, "mgs_scan_fps_batch: negative size%s");
  if (!cloud_size_ok(bucket_size))
    return fail(MGS_EINVAL, "mgs_scan_fps_batch: bucket_size must be positive and finite%s");
  if (ncloud == 0) return MGS_OK;
  if (!off || !k) return fail(MGS_EINVAL, "mgs_scan_fps_batch: null argument%s");
  if (off[0] != 0) return fail(MGS_EINVAL, "mgs_scan_fps_batch: off[0] must be 0%s");
  size_t ktot = 0;
  // first the offsets alone: only under ascending ones does every cloud lie inside points[0 .. 3 off[ncloud])
  for (int c = 0; c < ncloud; c++)
    if (off[c + 1] < off[c]) return fail_at(fail(MGS_EINVAL, "off must ascend%s"), E, "cloud", c);
  for (int c = 0; c < ncloud; c++) {
    if (int rc = scan_fps_check(points ? points + 3 * off[c] : nullptr, off[c + 1] - off[c], k[c], bucket_size, out_idx))
      return fail_at(rc, E, "cloud", c);
    ktot += (size_t)k[c];
  }
  if (ktot == 0) {
    if (out_nevals) for (int c = 0; c < ncloud; c++) out_nevals[c] = 0;
    return MGS_OK;
  }
  HIPCHK(hipSetDevice(device));
  DevBufs b;      // the points, the outputs and every cloud's pick set-up: until the pick has run
  double* dX = upload(b, points, 3 * (size_t)off[ncloud]);
  int32_t* dO = b.get<int32_t>(ktot);
  cloud_u64* dEv = b.get<cloud_u64>((size_t)ncloud);
  if (!b.ok) return fail(MGS_ENOMEM, "device allocation or upload failed%s");
  HIPCHK(hipMemsetAsync(dEv, 0, (size_t)ncloud * sizeof(cloud_u64), nullptr));
  EvTimer t;
  std::vector<CloudFpsJob> jobs;
  std::vector<int64_t> ns;
  size_t koff = 0;
  for (int c = 0; c < ncloud; c++) {
    if (k[c] == 0) continue;
    DevBufs s;      // this cloud's set-up scratch (its cell grid): released before the next cloud
    CloudFpsJob J;
    const int64_t n = off[c + 1] - off[c];
    int rc = cloud_fps_setup(s, b, dX + 3 * off[c], (int)n, k[c], bucket_size, dO + koff, dEv + c, &J);
    if (rc == MGS_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(MGS_EHIP, "HIP error in the pick's set-up%s");
    if (rc != MGS_OK) return fail_at(rc, E, "cloud", c);
    jobs.push_back(J);
    ns.push_back(n);
    koff += (size_t)k[c];
  }
  int rc = cloud_fps_launch_batch(b, jobs, ns, nullptr);
  if (rc != MGS_OK) return rc;
  rc = t.finish(kernel_ms);
  if (rc != MGS_OK) return rc;
  std::vector<cloud_u64> ev((size_t)ncloud);
  HIPCHK(hipMemcpy(ev.data(), dEv, (size_t)ncloud * sizeof(cloud_u64), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(out_idx, dO, ktot * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (out_nevals) for (int c = 0; c < ncloud; c++) out_nevals[c] = (int64_t)ev[c];
  return MGS_OK;
}

int mgs_scan_cloud_job_size(void) { return (int)sizeof(mgs_scan_cloud_job); }

int mgs_scan_cloud_batch(int device, int njob, mgs_scan_cloud_job* jobs, int nview, const double* cam_pos,
                         const double* cam_rot, int width, int height, double fx, double fy, double cx, double cy,
                         const double* extrinsics, double pfx, double pfy, double pcx, double pcy, int erode_iters,
                         const double* region, double voxel_size, double* pick_ms) {
  const char* E = "mgs_scan_cloud_batch";
  if (njob < 0) return fail(MGS_EINVAL, "mgs_scan_cloud_batch: negative size%s");
  CloudBatchViews v;
  if (int rc = scan_cloud_check_views(E, nview, cam_pos, cam_rot, width, height, fx, fy, extrinsics, pfx, pfy, erode_iters,
                                      voxel_size, &v.n))
    return rc;
  if (njob == 0) return MGS_OK;
  if (!jobs) return fail(MGS_EINVAL, "mgs_scan_cloud_batch: null argument%s");
  for (int j = 0; j < njob; j++)
    if (int rc = scan_cloud_check_scene(jobs[j].scene, jobs[j].colors, jobs[j].ncolor, jobs[j].num_points,
                                        jobs[j].out_points, jobs[j].out_colors))
      return fail_at(rc, E, "job", j);
  if (v.n == 0) {
    for (int j = 0; j < njob; j++) {
      jobs[j].out_n = 0;
      for (int i = 0; i < 8; i++) jobs[j].out_stats[i] = 0;
      for (int i = 0; i < 3; i++) jobs[j].stage_ms[i] = 0.0;
    }
    if (pick_ms) *pick_ms = 0.0;
    return MGS_OK;
  }
  HIPCHK(hipSetDevice(device));
  const size_t n = v.n;
  v.nview = nview, v.width = width, v.height = height, v.erode_iters = erode_iters;
  v.fx = fx, v.fy = fy, v.cx = cx, v.cy = cy, v.pfx = pfx, v.pfy = pfy, v.pcx = pcx, v.pcy = pcy;
  v.voxel_size = voxel_size;
  v.rg = region ? region : ref_region;
  DevBufs b;      // until the pick has run: the cameras, the images, every scene's voxels and pick set-up
  v.dCP = upload(b, cam_pos, 3 * (size_t)nview);
  v.dCR = upload(b, cam_rot, 9 * (size_t)nview);
  v.dE = upload(b, extrinsics, 16 * (size_t)nview);
  v.dD = b.get<double>(n);
  v.dD32 = b.get<double>(n);
  v.dS = b.get<int32_t>(n);
  v.dT = b.get<int32_t>(n);
  v.dN = b.get<int32_t>(n);
  v.dP = b.get<double>(3 * n);
  v.dK = b.get<uint8_t>(n);
  cloud_u64* dEv = b.get<cloud_u64>((size_t)njob);
  if (!b.ok) return fail(MGS_ENOMEM, "device allocation or upload failed%s");
  HIPCHK(hipMemsetAsync(dEv, 0, (size_t)njob * sizeof(cloud_u64), nullptr));
  std::vector<CloudBatchScene> held((size_t)njob);
  std::vector<CloudFpsJob> picks;
  std::vector<int64_t> pick_n;
  for (int j = 0; j < njob; j++) {
    bool picked = false;
    CloudFpsJob J;
    if (int rc = cloud_batch_scene(b, v, jobs[j], dEv + j, &held[j], &picked, &J)) return fail_at(rc, E, "job", j);
    if (picked) {
      picks.push_back(J);
      pick_n.push_back((int64_t)held[j].V.nvox);
    }
  }
  double ms = 0.0;
  if (int rc = cloud_fps_launch_batch(b, picks, pick_n, &ms)) return rc;
  for (int j = 0; j < njob; j++) {
    const CloudBatchScene& h = held[j];
    if (h.m > 0)
      hipLaunchKernelGGL(cloud_gather_kernel, dim3((h.m + MGS_CLOUD_BLOCK - 1) / MGS_CLOUD_BLOCK), dim3(MGS_CLOUD_BLOCK), 0,
                         nullptr, h.dIdx, h.m, h.V.vpts, h.V.vfeat, h.oP, h.oC);
  }
  HIPCHK(hipGetLastError());
  std::vector<cloud_u64> evals((size_t)njob);
  HIPCHK(hipMemcpy(evals.data(), dEv, (size_t)njob * sizeof(cloud_u64), hipMemcpyDeviceToHost));
  // every job has succeeded: only now is anything of the caller's written
  for (int j = 0; j < njob; j++) {
    const CloudBatchScene& h = held[j];
    if (h.m > 0) {
      HIPCHK(hipMemcpy(jobs[j].out_points, h.oP, 3 * (size_t)h.m * sizeof(float), hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(jobs[j].out_colors, h.oC, 3 * (size_t)h.m * sizeof(float), hipMemcpyDeviceToHost));
    }
  }
  for (int j = 0; j < njob; j++) {
    const CloudBatchScene& h = held[j];
    jobs[j].out_n = h.m;
    const int64_t stats[8] = {h.V.npts, h.V.nvox, (int64_t)evals[j], h.V.ncell, h.m, (int64_t)n, 0, 0};
    for (int i = 0; i < 8; i++) jobs[j].out_stats[i] = stats[i];
    for (int i = 0; i < 3; i++) jobs[j].stage_ms[i] = h.ms[i];
  }
  if (pick_ms) *pick_ms = ms;
  return MGS_OK;
}

// ---------------------------------------------------------------------------
// posed gripper cloud (csrc/mgs_pose.hip)
}  // extern "C"
namespace {
// everything of a pose call the host can check without the arrays' contents
int pose_check(const char* entry, const mgs_pose_tree* tree, int npoint, int nbatch, int ppg) {
  if (!tree) return fail(MGS_EINVAL, "%s: null tree", entry);
  if (tree->nlink < 1 || tree->nlink > MGS_POSE_MAXLINK) return fail(MGS_EINVAL, "%s: nlink must be 1 .. 32", entry);
  for (int i = 0; i < tree->nlink; i++)
    if (tree->parent[i] < -1 || tree->parent[i] >= i)
      return fail(MGS_EINVAL, "%s: parent[i] must lie in -1 .. i - 1", entry);
  if (npoint < 0 || nbatch < 0 || ppg < 0) return fail(MGS_EINVAL, "%s: negative size", entry);
  if (npoint > (1 << 30)) return fail(MGS_EINVAL, "%s: more than 2^30 points", entry);
  if (nbatch > 65535) return fail(MGS_EINVAL, "%s: at most 65535 joint states per call", entry);
  return MGS_OK;
}

// points per workgroup: whole tiles, and with few joint states enough groups
// for about four workgroups per CU of the device
int pose_group_size(int npoint, int nbatch, int ppg) {
  if (ppg > 0) return ppg;
  const int want = (1024 + nbatch - 1) / nbatch;      // groups per joint state
  int per = (npoint + want - 1) / want;
  per = (per + MGS_POSE_THREADS - 1) / MGS_POSE_THREADS * MGS_POSE_THREADS;
  return per < MGS_POSE_THREADS ? MGS_POSE_THREADS : per;
}

void pose_launch(const mgs_pose_tree* tree, int npoint, const double* dX, const int32_t* dL, int nbatch,
                 const double* dTh, const double* dB, int out_f32, void* dO, double* dW, int ppg, hipStream_t st) {
  const int per = pose_group_size(npoint, nbatch, ppg);
  const dim3 grid((unsigned)((npoint + per - 1) / per), (unsigned)nbatch);
  if (out_f32)
    hipLaunchKernelGGL(mgs_pose_cloud_kernel<float>, grid, dim3(MGS_POSE_THREADS), 0, st, *tree, npoint, dX, dL, dTh,
                       dB, (float*)dO, dW, per);
  else
    hipLaunchKernelGGL(mgs_pose_cloud_kernel<double>, grid, dim3(MGS_POSE_THREADS), 0, st, *tree, npoint, dX, dL, dTh,
                       dB, (double*)dO, dW, per);
}
}  // namespace
extern "C" {

int mgs_pose_tree_size(void) { return (int)sizeof(mgs_pose_tree); }

int mgs_pose_cloud(int device, const mgs_pose_tree* tree, int npoint, const double* points,
                   const int32_t* point_link, int nbatch, const double* theta, const double* base, int out_f32,
                   void* out_points, double* out_links, int points_per_group, double* kernel_ms) {
  if (int rc = pose_check("mgs_pose_cloud", tree, npoint, nbatch, points_per_group)) return rc;
  if (npoint > 0 && (!points || !point_link)) return fail(MGS_EINVAL, "mgs_pose_cloud: null argument%s");
  for (int p = 0; p < npoint; p++)
    if (point_link[p] < 0 || point_link[p] > tree->nlink)
      return fail(MGS_EINVAL, "mgs_pose_cloud: a point_link lies outside 0 .. nlink%s");
  if (kernel_ms) *kernel_ms = 0.0;
  if (npoint == 0 || nbatch == 0) return MGS_OK;
  if (!theta || !out_points) return fail(MGS_EINVAL, "mgs_pose_cloud: null argument%s");
  HIPCHK(hipSetDevice(device));
  const size_t np = (size_t)npoint, nb = (size_t)nbatch, nl = (size_t)tree->nlink;
  const size_t out_bytes = nb * np * 3 * (out_f32 ? sizeof(float) : sizeof(double));
  DevBufs b;
  double* dX = upload(b, points, 3 * np);
  int32_t* dL = upload(b, point_link, np);
  double* dTh = upload(b, theta, nb * nl);
  double* dB = base ? upload(b, base, 12 * nb) : nullptr;
  char* dO = b.get<char>(out_bytes);
  double* dW = out_links ? b.get<double>(nb * nl * 7) : nullptr;
  if (!b.ok) return fail(MGS_ENOMEM, "device allocation or upload failed%s");
  EvTimer t;
  pose_launch(tree, npoint, dX, dL, nbatch, dTh, dB, out_f32, dO, dW, points_per_group, nullptr);
  int rc = t.finish(kernel_ms);
  if (rc != MGS_OK) return rc;
  HIPCHK(hipMemcpy(out_points, dO, out_bytes, hipMemcpyDeviceToHost));
  if (out_links) HIPCHK(hipMemcpy(out_links, dW, nb * nl * 7 * sizeof(double), hipMemcpyDeviceToHost));
  return MGS_OK;
}

int mgs_pose_cloud_device(const mgs_pose_tree* tree, int npoint, const double* d_points, const int32_t* d_point_link,
                          int nbatch, const double* d_theta, const double* d_base, int out_f32, void* d_out_points,
                          double* d_out_links, int points_per_group, void* stream) {
  if (int rc = pose_check("mgs_pose_cloud_device", tree, npoint, nbatch, points_per_group)) return rc;
  if (npoint == 0 || nbatch == 0) return MGS_OK;
  if (!d_points || !d_point_link || !d_theta || !d_out_points)
    return fail(MGS_EINVAL, "mgs_pose_cloud_device: null argument%s");
  pose_launch(tree, npoint, d_points, d_point_link, nbatch, d_theta, d_base, out_f32, d_out_points, d_out_links,
              points_per_group, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MGS_OK;
}

int mgs_max_rows(void) { return 64 * MGS_RPL; }

int mgs_supports_nv(int nv) { return nv_supported(nv) ? 1 : 0; }

int mgs_rows_per_lane(void) { return MGS_RPL; }

int mgs_model_lds_bytes(const mgs_model_desc* desc, int64_t* out_bytes) {
  if (!desc || !out_bytes) return fail(MGS_EINVAL, "mgs_model_lds_bytes: null argument%s");
  size_t b = 0;
  make_layout(*desc, &b);
  *out_bytes = (int64_t)b;
  return MGS_OK;
}

int mgs_model_layout(const mgs_model_desc* desc, int32_t* out, int cap, int32_t* nwords) {
  if (!desc || !out || !nwords) return fail(MGS_EINVAL, "mgs_model_layout: null argument%s");
  size_t b = 0;
  if (cap < LAYOUT_WORDS) return fail(MGS_EINVAL, "mgs_model_layout: output too small%s");
  layout_words(make_layout(*desc, &b), out);
  *nwords = LAYOUT_WORDS;
  return MGS_OK;
}

int mgs_model_special(const mgs_model* m) { return m && m->special_rollout ? 1 : 0; }

int mgs_model_attach_special(mgs_model* m, const char* path) {
  if (!m || !path) return fail(MGS_EINVAL, "mgs_model_attach_special: null argument%s");
  HIPCHK(hipSetDevice(m->device));
  hipModule_t mod = nullptr;
  if (hipModuleLoad(&mod, path) != hipSuccess) return fail(MGS_EINVAL, "cannot load code object %s", path);
  // the object's baked ABI version, description and layout must be this model's
  auto check = [&]() -> int {
    // a global of a code object, read into *v when it has the expected size
    auto module_global = [](hipModule_t md, const char* name, void* v, size_t bytes) {
      hipDeviceptr_t p;
      size_t sz = 0;
      return hipModuleGetGlobal(&p, &sz, md, name) == hipSuccess && sz == bytes &&
             hipMemcpyDtoH(v, p, bytes) == hipSuccess;
    };
    auto module_int = [&](hipModule_t md, const char* name, int* v) { return module_global(md, name, v, sizeof(int)); };
    int abi = 0, rpl = 0, mxd = 0, mxnv = 0;
    mgs_model_desc dsc;
    int32_t w[LAYOUT_WORDS], mine[LAYOUT_WORDS];
    if (!module_int(mod, "mgs_special_abi", &abi) || abi != MGS_ABI_VERSION)
      return fail(MGS_EINVAL, "code object %s is of another ABI version", path);
    if (!module_int(mod, "mgs_special_rows_per_lane", &rpl) || rpl != MGS_RPL)
      return fail(MGS_EINVAL, "code object %s is of the other library flavour (rows per lane)", path);
    if (!module_int(mod, "mgs_special_maxdim", &mxd) || mxd != layout_maxdim(m->desc))
      return fail(MGS_EINVAL, "code object %s was built for another contact dimension (MGS_MAXDIM)", path);
    if (!module_int(mod, "mgs_special_max_nv", &mxnv) || mxnv < m->desc.nv)
      return fail(MGS_EINVAL, "code object %s holds fewer dofs per lane than the model needs (MGS_DPL)", path);
    if (!module_global(mod, "mgs_special_desc", &dsc, sizeof(dsc)) || memcmp(&dsc, &m->desc, sizeof(dsc)) != 0)
      return fail(MGS_EINVAL, "code object %s was specialised for another model description", path);
    layout_words(m->lay, mine);
    if (!module_global(mod, "mgs_special_words", w, sizeof(w)) || memcmp(w, mine, sizeof(w)) != 0)
      return fail(MGS_EINVAL, "code object %s was specialised for another LDS layout", path);
    return MGS_OK;
  };
  int rc = check();
  hipFunction_t fc = nullptr, fr = nullptr;
  // main-role objects name their kernels mgs_special_*, escalation-role ones
  // mgs_special_*_esc (mgs_special.hip).  The lookup of the naming an object
  // does not use fails by design: its error is cleared here, or the next
  // launch's hipGetLastError would report it
  if (rc == MGS_OK) {
    bool found = (hipModuleGetFunction(&fc, mod, "mgs_special_collision") == hipSuccess &&
                  hipModuleGetFunction(&fr, mod, "mgs_special_rollout") == hipSuccess) ||
                 (hipModuleGetFunction(&fc, mod, "mgs_special_collision_esc") == hipSuccess &&
                  hipModuleGetFunction(&fr, mod, "mgs_special_rollout_esc") == hipSuccess);
    (void)hipGetLastError();
    if (!found) rc = fail(MGS_EINVAL, "code object %s lacks the specialised kernels", path);
  }
  if (rc != MGS_OK) {
    hipModuleUnload(mod);
    return rc;
  }
  if (m->special_mod) hipModuleUnload(m->special_mod);
  m->special_mod = mod;
  m->special_collision = fc;
  m->special_rollout = fr;
  m->resident = 0;          // occupancy of the new rollout function, computed at its first launch
  return MGS_OK;
}

int mgs_rollout_grid(mgs_batch* b, int n) {
  if (!b || n < 0) return fail(MGS_EINVAL, "mgs_rollout_grid: bad argument%s");
  if (hipSetDevice(b->m->device) != hipSuccess) return fail(MGS_EHIP, "mgs_rollout_grid: hipSetDevice failed%s");
  const int r = queue_grid(b->m, n);
  return r ? r : n;
}

int mgs_rollout_queue(int mode) {
  int prev = queue_mode();
  if (mode >= 0) g_queue_mode = mode;
  return prev;
}

int mgs_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

}  // extern "C"
