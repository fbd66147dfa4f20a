// ebcsim.hip — C ABI of libebcsim.so (gfx950 / MI355X): handle, device buffers, launches.
// Kernels: ebc_kernels.h; device arithmetic: ebc_device.h, ebc_orca_group.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "ebc_host.h"
#include "ebc_dagger.h"
#include "ebc_group_sizes.h"
#include "ebc_kernels.h"
#include "ebc_local_map_kernel.h"
#include "ebc_mix_api.h"
#include "ebc_om_state.h"
#include "ebc_orca_wide_api.h"
#include "ebc_rollout.h"
#include "ebc_sail_api.h"
#include "ebc_world_api.h"

namespace {

using ebc::DevState;
using ebc::LookIO;
using ebc::StepIO;

using ebc_host::fail;
using ebc_host::g_err;

struct Handle {
  int device = 0;
  EbcParams p;
  DevState s;
  int T = 13;
  std::vector<void *> allocs;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  bool has_reset = false;
  double *act_scratch = nullptr;  // ebc_step_k: the ORCA robot's action when the caller keeps none
  // ebc_robot_sail: the attached network's packed weights (owned by the ebc_sail_create handle) and adult_num; the
  // per-step form's gathers of robot [E][9], ob [E][R][5] and the row counts [E], allocated on first use
  const float *sail_P = nullptr;
  int sail_N = 0;
  double *sail_robot = nullptr, *sail_ob = nullptr;
  long long *sail_rows = nullptr;
  int cus = 0;  // compute units of the device (EBC_FLAG_ONE_LAUNCH sizes its workgroups by them), read on first use
  int *robot_sim_rows = nullptr;
  ebc::RobotSim robot_sim = {nullptr, nullptr, nullptr};  // ebc_robot_orca_sim: the demonstrator's persistent rvo2 simulators
  bool faulted = false;  // a mailbox wait timed out and was reported: only ebc_reset re-arms the handle
  int orca_gs = 16;  // lanes per human of the ORCA waves
  unsigned epoch = 0;  // fused ORCA steps launched so far (StepGrid::epoch)
  std::vector<void *> pool_allocs;   // pool arrays (re-allocated by ebc_set_scene_pool)
  uint64_t *pool_grid_alloc = nullptr;
  // angular local map (ebc_local_map_config): polygons per scene slot, [E + P][S][4][2] and a count per slot
  bool lm_on = false;
  ebc::LocalMapCfg lm = {};
  double *lm_poly = nullptr;
  int *lm_npoly = nullptr;
  std::vector<uint8_t> lm_set;  // per slot: its polygons were written since the slot's scene was
  // staging for host-location calls
  void *stage = nullptr;
  size_t stage_bytes = 0;
  // timing
  bool timing = false;
  std::vector<hipEvent_t> ev;
  size_t ev_used = 0;
  double ms_sum = 0;
  int64_t launches = 0;
};

template <typename Tp>
int dev_alloc(Handle *h, Tp **out, size_t count) {
  void *ptr = nullptr;
  static const char *uncached = getenv("EBCSIM_UNCACHED_STATE");  // experiment: state the L2s do not hold
  if (uncached && uncached[0] == '1')
    HIP_TRY(hipExtMallocWithFlags(&ptr, count * sizeof(Tp) + 16, hipDeviceMallocUncached));
  else
    HIP_TRY(hipMalloc(&ptr, count * sizeof(Tp) + 16));
  HIP_TRY(hipMemset(ptr, 0, count * sizeof(Tp) + 16));
  h->allocs.push_back(ptr);
  *out = (Tp *)ptr;
  return EBC_OK;
}

int ensure_stage(Handle *h, size_t bytes) {
  if (bytes <= h->stage_bytes) return EBC_OK;
  if (h->stage) HIP_TRY(hipFree(h->stage));
  h->stage = nullptr;
  h->stage_bytes = 0;
  HIP_TRY(hipMalloc(&h->stage, bytes));
  h->stage_bytes = bytes;
  return EBC_OK;
}

// Mailboxes as every launch expects to find them (empty), and the fault word cleared.
int arm_mailboxes(Handle *h) {
  const size_t EN = (size_t)h->s.E * h->s.N, E = (size_t)h->s.E;
  // epoch tags of 0 match no launch (the epoch counter skips 0)
  HIP_TRY(hipMemsetAsync(h->s.vel, 0, EN * 16, h->stream));
  HIP_TRY(hipMemsetAsync(h->s.env_done, 0, E * 8, h->stream));
  HIP_TRY(hipMemsetAsync(h->s.rows_loaded, 0, E * 4, h->stream));
  HIP_TRY(hipMemsetAsync(h->s.robot_ready, 0, E * 4, h->stream));
  HIP_TRY(hipMemsetAsync(h->s.fault, 0, 4, h->stream));
  return EBC_OK;
}

// Called with the stream idle and the fault word's value in hand: a set word is reported ONCE
// (EBC_ERR_DEVICE), cleared, and the handle refuses further steps until ebc_reset re-arms it.
int report_fault(Handle *h, unsigned fault) {
  if (!fault) return EBC_OK;
  h->faulted = true;
  (void)hipMemset(h->s.fault, 0, 4);
  return fail(EBC_ERR_DEVICE, "ORCA step: a mailbox wait timed out; the state is undefined until ebc_reset");
}

// A bump allocator over the staging buffer for one host-location call.
struct Stager {
  Handle *h;
  size_t off = 0;
  struct Out { void *host; void *dev; size_t bytes; };
  std::vector<Out> outs;
  template <typename Tp>
  Tp *out(Tp *host, size_t count) {
    if (!host) return nullptr;
    Tp *d = (Tp *)((char *)h->stage + off);
    outs.push_back({(void *)host, (void *)d, count * sizeof(Tp)});
    off += (count * sizeof(Tp) + 255) & ~(size_t)255;
    return d;
  }
  template <typename Tp>
  int in(const Tp *host, size_t count, const Tp **dev) {
    *dev = nullptr;
    if (!host) return EBC_OK;
    Tp *d = (Tp *)((char *)h->stage + off);
    off += (count * sizeof(Tp) + 255) & ~(size_t)255;
    HIP_TRY(hipMemcpyAsync(d, host, count * sizeof(Tp), hipMemcpyHostToDevice, h->stream));
    *dev = d;
    return EBC_OK;
  }
  int finish() {
    for (auto &o : outs)
      HIP_TRY(hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, h->stream));
    unsigned fault = 0;  // rides with the copy-back: a host-location call never returns data of a broken step
    HIP_TRY(hipMemcpyAsync(&fault, h->s.fault, sizeof(fault), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return report_fault(h, fault);
  }
};

size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

int check_handle(void *handle, Handle **out) {
  if (!handle) return fail(EBC_ERR_INVALID, "null handle");
  *out = (Handle *)handle;
  hipError_t e = hipSetDevice((*out)->device);
  if (e != hipSuccess) return fail(EBC_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
  return EBC_OK;
}

int orca_blocks(const Handle *h) {
  const long humans = (long)h->s.E * h->s.N;
  const int hpw = EBC_WAVE / h->orca_gs;
  return (int)((humans + hpw - 1) / hpw);
}

// The ORCA group sizes (lanes per human, or per robot) the kernels are instantiated for.
const int kGroupSizes[] = {2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16, 21, 32};

// the smallest instantiated group size with at least n lanes (n <= 32)
int group_size_for(int n) {
  for (int g : kGroupSizes)
    if (g >= n) return g;
  return 32;
}

// the development builds' sizes and the run-time -> compile-time switch: ebc_group_sizes.h (shared with ebcsim_mix.hip)
using ebc_host::kDevHumanGs;
using ebc_host::kDevRobotGs;
using ebc_host::with_group_size;

int launch_orca(Handle *h) {
  const int blocks = orca_blocks(h);
  return with_group_size<kDevHumanGs>(h->orca_gs, [&](auto gs) -> int {
    hipLaunchKernelGGL((ebc::orca_kernel<decltype(gs)::value>), dim3(blocks), dim3(EBC_WAVE), 0, h->stream, h->p, h->s);
    HIP_TRY(hipGetLastError());
    return EBC_OK;
  });
}

template <int POLICY>
int launch_service(Handle *h, const StepIO &io) {
  const int epb = EBC_WAVE / h->s.N;
  const int blocks = (h->s.E + epb - 1) / epb;
  if (h->T == 17)
    hipLaunchKernelGGL((ebc::step_kernel<POLICY, 17>), dim3(blocks), dim3(EBC_WAVE), 0, h->stream, h->p, h->s, io);
  else
    hipLaunchKernelGGL((ebc::step_kernel<POLICY, 13>), dim3(blocks), dim3(EBC_WAVE), 0, h->stream, h->p, h->s, io);
  HIP_TRY(hipGetLastError());
  return EBC_OK;
}

// EBC_HUMAN_BY_TYPE: the mixed instantiation (ebcsim_mix.hip) with the arguments of launch_orca_step_gs
int launch_mixed_step(Handle *h, const StepIO &io, unsigned blocks, const ebc::StepGrid &g) {
  const void *kernel = nullptr;
  int rc = ebc_mix_api::step_kernel(h->orca_gs, h->T, &kernel);
  if (rc != EBC_OK) return rc;
  unsigned env_blocks = g.env_blocks, orca_blocks = g.orca_blocks, epoch = g.epoch, class_humans = g.ec * (unsigned)h->s.N;
  const float4 *tile = (const float4 *)h->s.tile;
  const int *n_humans = (const int *)h->s.n_humans;
  StepIO io_arg = io;
  ebc::StepGrid g_arg = g;
  void *args[] = {&env_blocks, &orca_blocks, &h->s.E, &h->s.N, &h->s.n_magic, &h->s.n_shift, &tile, &n_humans, &h->s.vel,
                  &epoch, &class_humans, &h->p, &h->s, &io_arg, &g_arg};
  HIP_TRY(hipLaunchKernel(kernel, dim3((blocks + EBC_STEP_WPB - 1) / EBC_STEP_WPB), dim3(EBC_WAVE * EBC_STEP_WPB), args, 0, h->stream));
  return EBC_OK;
}

template <int GS>
int launch_orca_step_gs(Handle *h, const StepIO &io, unsigned blocks, const ebc::StepGrid &g) {
  if (h->T == 17)
    hipLaunchKernelGGL((ebc::orca_step_kernel<GS, 17>), dim3((blocks + EBC_STEP_WPB - 1) / EBC_STEP_WPB), dim3(EBC_WAVE * EBC_STEP_WPB), 0, h->stream,
                       g.env_blocks, g.orca_blocks, h->s.E, h->s.N, h->s.n_magic, h->s.n_shift, (const float4 *)h->s.tile,
                       (const int *)h->s.n_humans, h->s.vel, g.epoch, g.ec * (unsigned)h->s.N, h->p, h->s, io, g);
  else
    hipLaunchKernelGGL((ebc::orca_step_kernel<GS, 13>), dim3((blocks + EBC_STEP_WPB - 1) / EBC_STEP_WPB), dim3(EBC_WAVE * EBC_STEP_WPB), 0, h->stream,
                       g.env_blocks, g.orca_blocks, h->s.E, h->s.N, h->s.n_magic, h->s.n_shift, (const float4 *)h->s.tile,
                       (const int *)h->s.n_humans, h->s.vel, g.epoch, g.ec * (unsigned)h->s.N, h->p, h->s, io, g);
  HIP_TRY(hipGetLastError());
  return EBC_OK;
}

int launch_orca_step(Handle *h, const StepIO &io, bool mixed = false) {
  // who does what: ebc_step_grid.h (eight classes of envs, every role a multiple of 8 blocks)
  const ebc::StepGridShape shape = ebc::step_grid_shape(h->s.E, h->s.N, h->s.S, h->orca_gs, io.ob || io.obs_rotated);
  if (!shape.fits()) return fail(EBC_ERR_UNSUPPORTED, "ORCA step grid >= 2^31 workgroups");
  const unsigned long long blocks = shape.total();
  ebc::StepGrid g;
  g.env_blocks = (unsigned)shape.env_blocks;
  g.orca_blocks = (unsigned)shape.orca_blocks;
  g.rows_blocks = (unsigned)shape.rows_blocks;
  g.rows_epw = shape.rows_epw;
  g.ec = shape.ec;
  if (++h->epoch == 0) h->epoch = 1;  // every mailbox word is tagged with the epoch of the launch that wrote it; 0 = never
  g.epoch = h->epoch;
  g.total = (unsigned)blocks;
  const int rc = mixed ? launch_mixed_step(h, io, (unsigned)blocks, g)
                       : with_group_size<kDevHumanGs>(
                             h->orca_gs, [&](auto gs) { return launch_orca_step_gs<decltype(gs)::value>(h, io, (unsigned)blocks, g); });
  // the launch leaves the robots' next state in robot_n and the humans' next positions in px_n / py_n: that is the
  // current state from here on (every other kernel and entry point reads and writes robot, px and py)
  if (rc == EBC_OK) {
    std::swap(h->s.robot, h->s.robot_n);
    std::swap(h->s.px, h->s.px_n);
    std::swap(h->s.py, h->s.py_n);
  }
  return rc;
}

int launch_step(Handle *h, const StepIO &io, int policy) {
  if (policy == EBC_HUMAN_ORCA) return launch_orca_step(h, io);
  if (policy == EBC_HUMAN_BY_TYPE) return launch_orca_step(h, io, true);
  if (policy == EBC_HUMAN_LINEAR) return launch_service<EBC_HUMAN_LINEAR>(h, io);
  return launch_service<EBC_HUMAN_EXTERNAL>(h, io);
}

template <int POLICY>
int launch_lookahead(Handle *h, const LookIO &io) {
  const size_t lds = (size_t)io.A * h->s.N * 8 + (io.rows ? (size_t)EBC_LA_THREADS * h->T * 4 : 0);
  if (h->T == 17)
    hipLaunchKernelGGL((ebc::lookahead_kernel<POLICY, 17>), dim3(h->s.E), dim3(EBC_LA_THREADS), lds, h->stream, h->p, h->s, io);
  else
    hipLaunchKernelGGL((ebc::lookahead_kernel<POLICY, 13>), dim3(h->s.E), dim3(EBC_LA_THREADS), lds, h->stream, h->p, h->s, io);
  HIP_TRY(hipGetLastError());
  return EBC_OK;
}

// Destination arrays of a scene upload: the live state or the scene pool.
struct SceneDst {
  int *n_humans;
  double *px, *py, *vx, *vy, *gx, *gy, *radius, *v_pref;
  uint8_t *type;
  int *n_static;
  double *spx, *spy, *sradius;
  uint64_t *grid;  // destination rows, written when the scene has a grid (or zeroed when `zero_grid`)
  double *robot;
};

// Pool arrays hold E reset slots + P custom scenes.  Re-allocation (ebc_set_scene_pool) keeps the
// reset slots.
int alloc_pool(Handle *h, int P) {
  ebc::ScenePool old = h->s.pool;
  std::vector<void *> old_allocs = h->pool_allocs;
  uint64_t *old_grid = h->pool_grid_alloc;
  h->pool_allocs.clear();
  ebc::ScenePool &pl = h->s.pool;
  const int E = h->s.E;
  const size_t slots = (size_t)E + P;
  const size_t PN = slots * h->s.N, PS = slots * (h->s.S ? h->s.S : 1);
  const size_t EN = (size_t)E * h->s.N, ES = (size_t)E * (h->s.S ? h->s.S : 1);
  const bool keep = !old_allocs.empty();
  auto get = [&](auto **out, size_t count, const void *from, size_t keep_count) -> int {
    void *ptr = nullptr;
    const size_t bytes = count * sizeof(**out) + 16;
    HIP_TRY(hipMalloc(&ptr, bytes));
    HIP_TRY(hipMemset(ptr, 0, bytes));
    if (keep && from) HIP_TRY(hipMemcpy(ptr, from, keep_count * sizeof(**out), hipMemcpyDeviceToDevice));
    h->pool_allocs.push_back(ptr);
    *out = reinterpret_cast<std::remove_reference_t<decltype(*out)>>(ptr);
    return EBC_OK;
  };
  int rc = EBC_OK;
#define G_(f, c, k) if (rc == EBC_OK) rc = get(&pl.f, (c), old.f, (k))
  G_(n_humans, slots, E); G_(px, PN, EN); G_(py, PN, EN); G_(vx, PN, EN); G_(vy, PN, EN); G_(gx, PN, EN);
  G_(gy, PN, EN); G_(radius, PN, EN); G_(v_pref, PN, EN); G_(type, PN, EN); G_(n_static, slots, E);
  G_(spx, PS, ES); G_(spy, PS, ES); G_(sradius, PS, ES); G_(robot, slots * 9, (size_t)E * 9);
  G_(pref, PN, EN);
#undef G_
  if (rc == EBC_OK) rc = get(&h->pool_grid_alloc, slots * h->s.G * 2, old_grid, (size_t)E * h->s.G * 2);
  pl.grid = (keep && old.grid) ? h->pool_grid_alloc : nullptr;
  pl.P = P;
  pl.stride = 0;
  pl.cursor = old.cursor;
  for (void *ptr : old_allocs) (void)hipFree(ptr);
  return rc;
}

// Copy rows of `sc` to rows `ids` (or 0..n-1) of `d`.
int upload_scene(Handle *h, const EbcScene *sc, const int32_t *ids, const SceneDst &d, bool with_grid,
                 hipMemcpyKind kind = hipMemcpyHostToDevice) {
  const int n = sc->n, N = h->s.N, S = h->s.S, G = h->s.G;
  bool contiguous = true;
  if (ids)
    for (int r = 0; r < n; ++r)
      if (ids[r] != ids[0] + r) contiguous = false;
  auto up = [&](void *dst_base, const void *src, size_t row_bytes) -> int {
    if (!src) return EBC_OK;
    if (contiguous) {
      const int e0 = ids ? ids[0] : 0;
      HIP_TRY(hipMemcpy((char *)dst_base + (size_t)e0 * row_bytes, src, (size_t)n * row_bytes, kind));
    } else {
      for (int r = 0; r < n; ++r)
        HIP_TRY(hipMemcpy((char *)dst_base + (size_t)ids[r] * row_bytes, (const char *)src + (size_t)r * row_bytes,
                          row_bytes, kind));
    }
    return EBC_OK;
  };
  int rc;
  const size_t rowN = (size_t)N * sizeof(double);
#define UP_(dst, src, bytes) if ((rc = up((void *)(dst), (const void *)(src), (bytes))) != EBC_OK) return rc
  UP_(d.n_humans, sc->n_humans, sizeof(int));
  UP_(d.px, sc->px, rowN); UP_(d.py, sc->py, rowN); UP_(d.vx, sc->vx, rowN); UP_(d.vy, sc->vy, rowN);
  UP_(d.gx, sc->gx, rowN); UP_(d.gy, sc->gy, rowN); UP_(d.radius, sc->radius, rowN);
  UP_(d.v_pref, sc->v_pref, rowN); UP_(d.type, sc->type, (size_t)N);
  UP_(d.robot, sc->robot, 9 * sizeof(double));
  if (S > 0) {
    UP_(d.n_static, sc->n_static, sizeof(int));
    UP_(d.spx, sc->spx, (size_t)S * sizeof(double)); UP_(d.spy, sc->spy, (size_t)S * sizeof(double));
    UP_(d.sradius, sc->sradius, (size_t)S * sizeof(double));
  }
  const size_t grow = (size_t)G * 2 * sizeof(uint64_t);
  if (sc->grid) {
    UP_(d.grid, sc->grid, grow);
  } else if (with_grid) {  // these rows get a free map
    const hipMemcpyKind scene_kind = kind;
    kind = hipMemcpyHostToDevice;
    std::vector<uint64_t> zeros((size_t)n * G * 2, 0);
    UP_(d.grid, zeros.data(), grow);
    kind = scene_kind;
  }
#undef UP_
  return EBC_OK;
}

int validate_scene(const Handle *h, const EbcScene *sc, const int32_t *ids, int id_limit) {
  const int N = h->s.N, S = h->s.S;
  if (!sc || sc->struct_size != sizeof(EbcScene)) return fail(EBC_ERR_INVALID, "EbcScene.struct_size");
  if (sc->n <= 0) return fail(EBC_ERR_INVALID, "scene.n");
  if (!sc->n_humans || !sc->px || !sc->py || !sc->vx || !sc->vy || !sc->gx || !sc->gy || !sc->radius ||
      !sc->v_pref || !sc->type || !sc->robot)
    return fail(EBC_ERR_INVALID, "scene array missing");
  if (S > 0 && (!sc->n_static || !sc->spx || !sc->spy || !sc->sradius))
    return fail(EBC_ERR_INVALID, "static rows missing");
  for (int r = 0; r < sc->n; ++r) {  // what the kernels assume, checked on the host
    const int e = ids ? ids[r] : r;
    if (e < 0 || e >= id_limit) return fail(EBC_ERR_INVALID, "env id out of range");
    if (sc->n_humans[r] < 0 || sc->n_humans[r] > N) return fail(EBC_ERR_INVALID, "n_humans > max_humans");
    if (S > 0 && (sc->n_static[r] < 0 || sc->n_static[r] > S)) return fail(EBC_ERR_INVALID, "n_static > max_static");
    for (int i = 0; i < sc->n_humans[r]; ++i)
      if (sc->type[(size_t)r * N + i] > EBC_CHILD) return fail(EBC_ERR_INVALID, "human type must be 0..2");
  }
  return EBC_OK;
}

// ---- angular local map storage: slot r of [E + P] holds r's polygons at lm_poly + r * S1 * 8
size_t lm_s1(const Handle *h) { return h->s.S ? (size_t)h->s.S : 1; }

// (Re)allocate the polygon storage for E + P slots, keeping the first `keep` slots' contents and marks.
int lm_alloc(Handle *h, int slots, int keep) {
  double *poly = nullptr;
  int *npoly = nullptr;
  const size_t S1 = lm_s1(h);
  HIP_TRY(hipMalloc(&poly, (size_t)slots * S1 * 8 * sizeof(double) + 16));
  HIP_TRY(hipMalloc(&npoly, (size_t)slots * sizeof(int) + 16));
  HIP_TRY(hipMemset(npoly, 0, (size_t)slots * sizeof(int) + 16));
  if (keep > 0 && h->lm_poly) {
    HIP_TRY(hipMemcpy(poly, h->lm_poly, (size_t)keep * S1 * 8 * sizeof(double), hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(npoly, h->lm_npoly, (size_t)keep * sizeof(int), hipMemcpyDeviceToDevice));
  }
  if (h->lm_poly) (void)hipFree(h->lm_poly);
  if (h->lm_npoly) (void)hipFree(h->lm_npoly);
  h->lm_poly = poly;
  h->lm_npoly = npoly;
  h->lm_set.resize((size_t)slots, 0);
  for (size_t r = (size_t)keep; r < h->lm_set.size(); ++r) h->lm_set[r] = 0;
  return EBC_OK;
}

// Polygons rows -> slots (slot of row r = slots[r], or first + r); kind: where `poly` / `npoly` live.
int lm_upload(Handle *h, const int *slots, int first, int n, const double *poly, const int *npoly, hipMemcpyKind kind) {
  const size_t row = lm_s1(h) * 8 * sizeof(double);
  if (!slots) {
    HIP_TRY(hipMemcpy((char *)h->lm_poly + (size_t)first * row, poly, (size_t)n * row, kind));
    HIP_TRY(hipMemcpy(h->lm_npoly + first, npoly, (size_t)n * sizeof(int), kind));
  } else {
    for (int r = 0; r < n; ++r) {
      HIP_TRY(hipMemcpy((char *)h->lm_poly + (size_t)slots[r] * row, (const char *)poly + (size_t)r * row, row, kind));
      HIP_TRY(hipMemcpy(h->lm_npoly + slots[r], npoly + r, sizeof(int), kind));
    }
  }
  for (int r = 0; r < n; ++r) h->lm_set[(size_t)(slots ? slots[r] : first + r)] = 1;
  return EBC_OK;
}

// Every slot an env can reach holds polygons: its own ebc_reset slot and every pool scene.
int lm_ready(const Handle *h, const char *what) {
  if (!h->lm_on) return fail(EBC_ERR_STATE, std::string(what) + " before ebc_local_map_config");
  if (h->s.S == 0) return EBC_OK;  // no scene of this handle can hold an obstacle
  const int E = h->s.E;
  for (int e = 0; e < E; ++e)
    if (!h->lm_set[(size_t)e])
      return fail(EBC_ERR_STATE, std::string(what) + ": env " + std::to_string(e) +
                                     " has no obstacles for its ebc_reset scene (ebc_set_obstacles)");
  for (size_t r = (size_t)E; r < h->lm_set.size(); ++r)
    if (!h->lm_set[r])
      return fail(EBC_ERR_STATE, std::string(what) + ": pool scene " + std::to_string(r - E) +
                                     " has no obstacles (ebc_set_obstacle_pool)");
  return EBC_OK;
}

int launch_local_map(Handle *h, int next, int robot_policy, const double *robot_action, double *out) {
  ebc::LocalMapIO io;
  io.c = h->lm;
  io.poly = h->lm_poly;
  io.n_poly = h->lm_npoly;
  io.S = (int)lm_s1(h);
  io.next = next;
  io.robot_policy = robot_policy;
  io.robot_action = robot_action;
  io.out = out;
  hipLaunchKernelGGL(ebc::local_map_kernel, dim3((unsigned)h->s.E), dim3(EBC_WAVE), 0, h->stream, h->p, h->s, io);
  HIP_TRY(hipGetLastError());
  return EBC_OK;
}

}  // namespace

extern "C" {

int ebc_abi_version(void) { return EBC_ABI_VERSION; }

const char *ebc_last_error(void) { return g_err.c_str(); }

int ebc_params_default(EbcParams *p) {
  if (!p) return fail(EBC_ERR_INVALID, "null params");
  memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(EbcParams);
  p->robot_kinematics = EBC_HOLONOMIC;
  p->time_step = 0.25;
  p->time_limit = 25;
  p->map_size_m = 9.0;
  p->map_resolution = 0.1;
  p->time_max = NAN;
  p->time_good = 10.0;
  p->max_goal_distance = NAN;
  p->success_reward = 1.0;
  for (int i = 0; i < 4; ++i) p->collision_penalty[i] = NAN;
  for (int i = 0; i < 3; ++i) {
    p->discomfort_dist[i] = 0.1;
    p->discomfort_factor[i] = 0.5;
  }
  p->orca_neighbor_dist = 10.0f;
  p->orca_time_horizon = 5.0f;
  p->orca_max_neighbors = 10;
  return EBC_OK;
}

int ebc_create(int device_id, int n_envs, int max_humans, int max_static, const EbcParams *params,
               void **handle_out) {
  if (!params || !handle_out) return fail(EBC_ERR_INVALID, "null argument");
  if (params->struct_size != sizeof(EbcParams))
    return fail(EBC_ERR_INVALID, "EbcParams.struct_size does not match this library");
  if (n_envs <= 0 || max_humans <= 0 || max_static < 0) return fail(EBC_ERR_INVALID, "bad dimensions");
  if ((double)n_envs * max_humans >= 2147483648.0) return fail(EBC_ERR_UNSUPPORTED, "n_envs * max_humans >= 2^31");
  if (max_humans - 1 + (params->robot_visible ? 1 : 0) > 32)
    return fail(EBC_ERR_UNSUPPORTED, "more than 32 other agents per human (ORCA group of 32 lanes)");
  if (max_humans + max_static > EBC_LA_MAX_ROWS)
    return fail(EBC_ERR_UNSUPPORTED, "max_humans + max_static > 128 observation rows");
  if (params->orca_max_neighbors > EBC_MAXNB || params->orca_max_neighbors < 0)
    return fail(EBC_ERR_UNSUPPORTED, "orca_max_neighbors > 10");
  if (params->robot_kinematics != EBC_HOLONOMIC && params->robot_kinematics != EBC_UNICYCLE)
    return fail(EBC_ERR_INVALID, "robot_kinematics");
  const int G = (int)std::nearbyint(params->map_size_m / params->map_resolution);
  if (G <= 0 || G > 128) return fail(EBC_ERR_UNSUPPORTED, "occupancy grid wider than 128 cells");
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(EBC_ERR_DEVICE, "no HIP device: libebcsim has no CPU fallback");
  if (device_id < 0 || device_id >= count) return fail(EBC_ERR_INVALID, "device_id out of range");
  HIP_TRY(hipSetDevice(device_id));
  Handle *h = new Handle();
  h->device = device_id;
  h->p = *params;
  h->T = params->with_agent_type ? 17 : 13;
  DevState &s = h->s;
  memset(&s, 0, sizeof(s));
  s.E = n_envs;
  s.N = max_humans;
  s.S = max_static;
  s.G = G;
  // rvo2 holds these as floats (Agent.cpp: invTimeHorizon, invTimeStep, rangeSq)
  s.inv_time_horizon = 1.0f / params->orca_time_horizon;
  s.inv_time_step = 1.0f / (float)params->time_step;
  s.range_sq = params->orca_neighbor_dist * params->orca_neighbor_dist;
  {  // h / N for h < 2^31 as mulhi(h, magic) >> shift (N >= 2; N == 1 is the identity)
    unsigned sh = 0;
    while ((1u << sh) < (unsigned)max_humans) ++sh;
    s.n_magic = max_humans > 1 ? (unsigned)((1ull << (31 + sh)) / (unsigned)max_humans + 1) : 0;
    s.n_shift = max_humans > 1 ? sh - 1 : 0;
  }
  const size_t EN = (size_t)n_envs * max_humans, ES = (size_t)n_envs * (max_static ? max_static : 1);
  int rc = EBC_OK;
#define A_(field, cnt) if (rc == EBC_OK) rc = dev_alloc(h, &s.field, (cnt))
  A_(n_humans, n_envs); A_(px, EN); A_(py, EN); A_(px_n, EN); A_(py_n, EN); A_(vx, EN); A_(vy, EN); A_(gx, EN); A_(gy, EN);
  A_(radius, EN); A_(v_pref, EN); A_(type, EN); A_(n_static, n_envs); A_(spx, ES); A_(spy, ES);
  A_(sradius, ES); A_(robot, (size_t)n_envs * 9); A_(robot_n, (size_t)n_envs * 9); A_(time, n_envs); A_(arrival, EN);
  A_(tile, EN * 2);
  A_(done, n_envs); A_(hact, EN * 2);
  A_(vel, 2 * EN);  // the words, then the linear boxes of EBC_HUMAN_BY_TYPE (linear_box, ebc_kernels.h)
  A_(env_done, n_envs); A_(rows_loaded, n_envs); A_(robot_ready, n_envs); A_(fault, 1);  // zeroed: tag 0 = no launch
#undef A_
  if (rc == EBC_OK) rc = dev_alloc(h, &s.pool.cursor, n_envs);
  if (rc == EBC_OK) rc = dev_alloc(h, &s.grid_scene, n_envs);
  if (rc == EBC_OK) rc = alloc_pool(h, 0);
  if (rc != EBC_OK) {
    for (void *ptr : h->allocs) (void)hipFree(ptr);
    delete h;
    return rc;
  }
  if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) {
    for (void *ptr : h->allocs) (void)hipFree(ptr);
    delete h;
    return fail(EBC_ERR_DEVICE, "hipStreamCreate failed");
  }
  h->stream = h->own_stream;
  {
    const int others = max_humans - 1 + (params->robot_visible ? 1 : 0);
    // lanes per human = its number of others, rounded up to a size that is instantiated and never
    // to one that fits fewer humans in a wave (64 / GS): 9 others -> 9 lanes, 7 humans per wave
    h->orca_gs = group_size_for(others);
    const char *force = getenv("EBCSIM_ORCA_GROUP");  // measurements only: a larger group size
    if (force && atoi(force) >= h->orca_gs && atoi(force) <= 32) h->orca_gs = group_size_for(atoi(force));
  }
  *handle_out = h;
  return EBC_OK;
}

int ebc_destroy(void *handle) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  (void)hipStreamSynchronize(h->stream);
  for (void *ptr : h->allocs) (void)hipFree(ptr);
  for (void *ptr : h->pool_allocs) (void)hipFree(ptr);
  if (h->lm_poly) (void)hipFree(h->lm_poly);
  if (h->lm_npoly) (void)hipFree(h->lm_npoly);
  if (h->stage) (void)hipFree(h->stage);
  for (hipEvent_t ev : h->ev) (void)hipEventDestroy(ev);
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  delete h;
  return EBC_OK;
}

int ebc_set_stream(void *handle, void *hip_stream) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->stream = (hipStream_t)hip_stream;  // NULL = the HIP null stream (torch's default stream)
  return EBC_OK;
}

int ebc_synchronize(void *handle) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  unsigned fault = 0;  // a role of the fused ORCA step gave up waiting for another (never expected)
  HIP_TRY(hipMemcpy(&fault, h->s.fault, sizeof(fault), hipMemcpyDeviceToHost));
  return report_fault(h, fault);
}

int ebc_dims(void *handle, int32_t out[5]) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  out[0] = h->s.E; out[1] = h->s.N; out[2] = h->s.S; out[3] = h->T; out[4] = h->s.G;
  return EBC_OK;
}

// env.reset of the listed envs from `sc`, whose arrays are on the host (ebc_reset) or on the device (ebc_generate_reset)
static int reset_impl(Handle *h, const int32_t *env_ids, const EbcScene *sc, hipMemcpyKind kind) {
  int rc;
  DevState &s = h->s;
  const int n = sc->n, N = s.N;
  if (n > s.E) return fail(EBC_ERR_INVALID, "scene.n out of range");
  HIP_TRY(hipStreamSynchronize(h->stream));
  ebc::ScenePool &pl = s.pool;
  if (sc->grid) pl.grid = h->pool_grid_alloc;
  // the live state ...
  const SceneDst live = {s.n_humans, s.px, s.py, s.vx, s.vy, s.gx, s.gy, s.radius, s.v_pref, s.type,
                         s.n_static, s.spx, s.spy, s.sradius, nullptr, s.robot};
  EbcScene no_grid = *sc;
  no_grid.grid = nullptr;
  if ((rc = upload_scene(h, &no_grid, env_ids, live, false, kind)) != EBC_OK) return rc;
  // ... and reset slot e of the pool (auto-reset source, and the home of env e's occupancy grid)
  const SceneDst slot = {pl.n_humans, pl.px, pl.py, pl.vx, pl.vy, pl.gx, pl.gy, pl.radius, pl.v_pref,
                         pl.type, pl.n_static, pl.spx, pl.spy, pl.sradius, h->pool_grid_alloc, pl.robot};
  if ((rc = upload_scene(h, sc, env_ids, slot, pl.grid != nullptr, kind)) != EBC_OK) return rc;
  // per-env scalars: global_time = 0, arrival = 0, done = 0 (env.py:149-151); grid and restart slot
  bool contiguous = true;
  for (int r = 0; r < n && env_ids; ++r)
    if (env_ids[r] != env_ids[0] + r) contiguous = false;
  std::vector<int> ids(n);
  for (int r = 0; r < n; ++r) ids[r] = env_ids ? env_ids[r] : r;
  const size_t rowN = (size_t)N * sizeof(double);
  if (contiguous) {
    const int e0 = ids[0];
    HIP_TRY(hipMemset(s.time + e0, 0, (size_t)n * sizeof(double)));
    HIP_TRY(hipMemset(s.arrival + (size_t)e0 * N, 0, (size_t)n * rowN));
    HIP_TRY(hipMemset(s.done + e0, 0, (size_t)n));
    HIP_TRY(hipMemcpy(s.grid_scene + e0, ids.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    if (pl.P == 0) HIP_TRY(hipMemcpy(pl.cursor + e0, ids.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  } else {
    for (int r = 0; r < n; ++r) {
      const int e = ids[r];
      HIP_TRY(hipMemset(s.time + e, 0, sizeof(double)));
      HIP_TRY(hipMemset(s.arrival + (size_t)e * N, 0, rowN));
      HIP_TRY(hipMemset(s.done + e, 0, 1));
      HIP_TRY(hipMemcpy(s.grid_scene + e, &e, sizeof(int), hipMemcpyHostToDevice));
      if (pl.P == 0) HIP_TRY(hipMemcpy(pl.cursor + e, &e, sizeof(int), hipMemcpyHostToDevice));
    }
  }
  {  // the float tile the ORCA waves read (orca.py:110-140), for the whole batch, and the preferred
     // velocities of the reset slots
    const size_t EN = (size_t)s.E * N;
    hipLaunchKernelGGL(ebc::pool_pref_kernel, dim3((unsigned)((EN + 255) / 256)), dim3(256), 0, h->stream, h->s, (size_t)0, EN);
    hipLaunchKernelGGL(ebc::tile_kernel, dim3((unsigned)((EN + 255) / 256)), dim3(256), 0, h->stream, h->p, h->s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  // between launches every mailbox is empty; after a reported fault they may not be: re-arm
  if (h->faulted) {
    if ((rc = arm_mailboxes(h)) != EBC_OK) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->faulted = false;
  }
  if (h->lm_on)  // the scenes changed: their polygons come with ebc_set_obstacles (or the generator)
    for (int r = 0; r < n; ++r) h->lm_set[(size_t)ids[r]] = 0;
  h->has_reset = true;
  return EBC_OK;
}

int ebc_reset(void *handle, const int32_t *env_ids, const EbcScene *sc) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  if ((rc = validate_scene(h, sc, env_ids, h->s.E)) != EBC_OK) return rc;
  return reset_impl(h, env_ids, sc, hipMemcpyHostToDevice);
}

static int pool_impl(Handle *h, const EbcScene *sc, int stride, hipMemcpyKind kind) {
  int rc;
  DevState &s = h->s;
  if (stride < 0) return fail(EBC_ERR_INVALID, "stride");
  HIP_TRY(hipStreamSynchronize(h->stream));
  const int P = sc->n, E = s.E;
  bool old_pool_set = true;  // every polygon a running env can be moved from is known
  for (size_t r = (size_t)E; h->lm_on && r < h->lm_set.size(); ++r) old_pool_set = old_pool_set && h->lm_set[r];
  if (h->has_reset) {  // running episodes keep their maps: into the envs' own slots before the old slots are freed
    if (h->lm_on)  // the polygons first: rehome_grid_kernel rewrites grid_scene
      hipLaunchKernelGGL(ebc::rehome_poly_kernel, dim3((unsigned)E), dim3(64), 0, h->stream, h->s, h->lm_poly, h->lm_npoly,
                         (int)lm_s1(h));
    hipLaunchKernelGGL(ebc::rehome_grid_kernel, dim3((unsigned)E), dim3(256), 0, h->stream, h->s, h->pool_grid_alloc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  if ((rc = alloc_pool(h, P)) != EBC_OK) return rc;  // keeps the E reset slots
  if (h->lm_on) {  // so does the polygon storage; the pool's polygons are unset until written
    if ((rc = lm_alloc(h, E + P, E)) != EBC_OK) return rc;
    if (!old_pool_set)
      for (int e = 0; e < E; ++e) h->lm_set[(size_t)e] = 0;
  }
  ebc::ScenePool &pl = s.pool;
  if (sc->grid) pl.grid = h->pool_grid_alloc;
  const size_t N = s.N, S = s.S ? s.S : 1;
  const SceneDst slot = {pl.n_humans + E, pl.px + E * N, pl.py + E * N, pl.vx + E * N, pl.vy + E * N,
                         pl.gx + E * N, pl.gy + E * N, pl.radius + E * N, pl.v_pref + E * N, pl.type + E * N,
                         pl.n_static + E, pl.spx + E * S, pl.spy + E * S, pl.sradius + E * S,
                         h->pool_grid_alloc + (size_t)E * s.G * 2, pl.robot + (size_t)E * 9};
  if ((rc = upload_scene(h, sc, nullptr, slot, false, kind)) != EBC_OK) return rc;
  {
    const size_t first = (size_t)E * N, count = (size_t)P * N;
    hipLaunchKernelGGL(ebc::pool_pref_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, h->s, first, count);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  pl.stride = stride % P;
  std::vector<int> cur(E);
  for (int e = 0; e < E; ++e) cur[e] = E + e % P;
  HIP_TRY(hipMemcpy(pl.cursor, cur.data(), (size_t)E * sizeof(int), hipMemcpyHostToDevice));
  return EBC_OK;
}

int ebc_set_scene_pool(void *handle, const EbcScene *sc, int stride) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  if ((rc = validate_scene(h, sc, nullptr, sc ? sc->n : 0)) != EBC_OK) return rc;
  return pool_impl(h, sc, stride, hipMemcpyHostToDevice);
}

// ---- scenes generated on the device (ebc_scene_gen.h)
namespace {
struct GenBatch {  // n generated scenes in device memory, freed with the object
  std::vector<void *> allocs;
  EbcScene sc;  // device pointers
  double *poly = nullptr;  // [n][S][4][2] and [n]: written when local maps are configured
  int *n_poly = nullptr;
  ~GenBatch() {
    for (void *ptr : allocs) (void)hipFree(ptr);
  }
};

int validate_gen(const Handle *h, const EbcSceneGen *g, int n) {
  if (!g || g->struct_size != sizeof(EbcSceneGen)) return fail(EBC_ERR_INVALID, "EbcSceneGen.struct_size");
  if (n <= 0) return fail(EBC_ERR_INVALID, "number of scenes");
  long total = 0;
  for (int t = 0; t < 3; ++t) {
    if (g->count[t] < 0) return fail(EBC_ERR_INVALID, "EbcSceneGen.count");
    const int r = g->rule[t];
    // the crowd rules place a number of adults of their own whatever count[0] says (scene_generator.py:523-589);
    // the generator asks the same function, so a code that is no crowd rule here places count[t] humans there
    const int crowd = ebc::crowd_capacity(r);
    if (crowd && t != EBC_ADULT)
      return fail(EBC_ERR_INVALID, r == EBC_RULE_MIXED      ? "the mixed rule is defined for adults only"
                                   : r == EBC_RULE_MIXED_20 ? "the mixed_20 rule is defined for adults only"
                                                            : "the one_static rule is defined for adults only");
    total += crowd ? crowd : g->count[t];
    if (crowd || !g->count[t]) continue;
    if (r != EBC_RULE_CIRCLE_CROSSING && r != EBC_RULE_SQUARE_CROSSING && r != EBC_RULE_SQUARE_CROSSING_OLD)
      return fail(EBC_ERR_INVALID, "EbcSceneGen.rule");
    // what the reference itself cannot run (scene_generator.py:449-457 raises for children on the circle; the
    // old square rule exists for bicycles only, :459-498)
    if (r == EBC_RULE_CIRCLE_CROSSING && t == EBC_CHILD) return fail(EBC_ERR_INVALID, "circle_crossing is not defined for children");
    if (r == EBC_RULE_SQUARE_CROSSING_OLD && t != EBC_BICYCLE) return fail(EBC_ERR_INVALID, "square_crossing_old is defined for bicycles only");
  }
  if (total > h->s.N) return fail(EBC_ERR_INVALID, "the generated scenes have more humans than max_humans");
  if (g->num_circles < 0 || g->num_walls < 0) return fail(EBC_ERR_INVALID, "EbcSceneGen.num_circles / num_walls");
  if (g->num_walls > 0 && (g->min_wall_length < 1 || g->max_wall_length < g->min_wall_length))
    return fail(EBC_ERR_INVALID, "EbcSceneGen.min_wall_length / max_wall_length");
  if (!(g->map_resolution > 0) || (int)std::nearbyint(g->map_size_m / g->map_resolution) != h->s.G)
    return fail(EBC_ERR_INVALID, "EbcSceneGen map size differs from the handle's");
  if (g->num_circles + g->num_walls > 0 && h->s.S == 0)
    return fail(EBC_ERR_INVALID, "a map with obstacles needs max_static > 0");
  return EBC_OK;
}

int generate_batch(Handle *h, const EbcSceneGen *gen, uint32_t seed0, const uint32_t *seeds, int n, GenBatch &b) {
  int rc = validate_gen(h, gen, n);
  if (rc) return rc;
  const int N = h->s.N, S = h->s.S, G = h->s.G;
  const size_t nN = (size_t)n * N, nS = (size_t)n * (S ? S : 1);
  auto get = [&](auto **out, size_t count) -> int {
    void *ptr = nullptr;
    HIP_TRY(hipMalloc(&ptr, count * sizeof(**out) + 16));
    b.allocs.push_back(ptr);
    *out = reinterpret_cast<std::remove_reference_t<decltype(*out)>>(ptr);
    return EBC_OK;
  };
  ebc::SceneRow d = {};
  uint32_t *mt = nullptr, *dseeds = nullptr;
  int *status = nullptr;
  const bool with_grid = gen->num_circles + gen->num_walls > 0;
#define G_(f, c) if (rc == EBC_OK) rc = get(&d.f, (c))
  G_(n_humans, n); G_(px, nN); G_(py, nN); G_(vx, nN); G_(vy, nN); G_(gx, nN); G_(gy, nN); G_(radius, nN); G_(v_pref, nN);
  G_(type, nN); G_(n_static, n); G_(spx, nS); G_(spy, nS); G_(sradius, nS); G_(robot, (size_t)n * 9);
  if (with_grid) G_(grid, (size_t)n * G * 2);
  if (h->lm_on && S > 0) {
    G_(poly, nS * 8);
    G_(n_poly, n);
  }
#undef G_
  if (rc == EBC_OK) rc = get(&mt, (size_t)n * 624);
  if (rc == EBC_OK) rc = get(&status, 1);
  if (rc == EBC_OK && seeds) rc = get(&dseeds, n);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(status, 0, sizeof(int), h->stream));
  if (!S) {  // one placeholder row per scene that the kernel has no reason to write: ebc_generate_scenes copies it out
    HIP_TRY(hipMemsetAsync(d.spx, 0, nS * sizeof(double), h->stream));
    HIP_TRY(hipMemsetAsync(d.spy, 0, nS * sizeof(double), h->stream));
    HIP_TRY(hipMemsetAsync(d.sradius, 0, nS * sizeof(double), h->stream));
  }
  if (seeds) HIP_TRY(hipMemcpyAsync(dseeds, seeds, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(ebc::scene_gen_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, h->stream, *gen, (const uint32_t *)dseeds,
                     seed0, n, N, S, G, d, mt, status);
  HIP_TRY(hipGetLastError());
  int st = 0;
  HIP_TRY(hipMemcpyAsync(&st, status, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (st & EBC_GEN_STATIC_OVERFLOW) return fail(EBC_ERR_INVALID, "a generated map has more observation rows than max_static");
  EbcScene &sc = b.sc;
  memset(&sc, 0, sizeof(sc));
  sc.struct_size = sizeof(EbcScene);
  sc.n = n;
  sc.n_humans = d.n_humans;
  sc.px = d.px; sc.py = d.py; sc.vx = d.vx; sc.vy = d.vy; sc.gx = d.gx; sc.gy = d.gy; sc.radius = d.radius; sc.v_pref = d.v_pref;
  sc.type = d.type;
  sc.n_static = d.n_static;
  sc.spx = d.spx; sc.spy = d.spy; sc.sradius = d.sradius;
  sc.grid = d.grid;
  sc.robot = d.robot;
  b.poly = d.poly;
  b.n_poly = d.n_poly;
  return EBC_OK;
}
}  // namespace

int ebc_generate_scenes(void *handle, const EbcSceneGen *gen, uint32_t seed0, const uint32_t *seeds, int n, EbcSceneOut *out) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  if (!out || out->struct_size != sizeof(EbcSceneOut)) return fail(EBC_ERR_INVALID, "EbcSceneOut.struct_size");
  GenBatch b;
  if ((rc = generate_batch(h, gen, seed0, seeds, n, b)) != EBC_OK) return rc;
  const hipMemcpyKind kind = out->location == EBC_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const size_t N = h->s.N, S = h->s.S ? h->s.S : 1, G = h->s.G;
  const EbcScene &sc = b.sc;
#define OUT_(f, bytes) if (out->f && sc.f) HIP_TRY(hipMemcpy(out->f, sc.f, (size_t)n * (bytes), kind))
  OUT_(n_humans, sizeof(int)); OUT_(px, N * 8); OUT_(py, N * 8); OUT_(vx, N * 8); OUT_(vy, N * 8); OUT_(gx, N * 8); OUT_(gy, N * 8);
  OUT_(radius, N * 8); OUT_(v_pref, N * 8); OUT_(type, N); OUT_(n_static, sizeof(int)); OUT_(spx, S * 8); OUT_(spy, S * 8);
  OUT_(sradius, S * 8); OUT_(robot, 72); OUT_(grid, G * 16);
#undef OUT_
  if (out->grid && !sc.grid) {  // free maps
    if (out->location == EBC_DEVICE) HIP_TRY(hipMemset(out->grid, 0, (size_t)n * G * 16));
    else memset(out->grid, 0, (size_t)n * G * 16);
  }
  return EBC_OK;
}

int ebc_generate_reset(void *handle, const EbcSceneGen *gen, uint32_t seed0, const uint32_t *seeds, int first, int n) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  if (first < 0 || n <= 0 || (long)first + n > h->s.E) return fail(EBC_ERR_INVALID, "env range");
  GenBatch b;
  if ((rc = generate_batch(h, gen, seed0, seeds, n, b)) != EBC_OK) return rc;
  std::vector<int32_t> ids(n);
  for (int r = 0; r < n; ++r) ids[r] = first + r;
  if ((rc = reset_impl(h, ids.data(), &b.sc, hipMemcpyDeviceToDevice)) != EBC_OK) return rc;
  if (b.poly) return lm_upload(h, nullptr, first, n, b.poly, b.n_poly, hipMemcpyDeviceToDevice);
  return EBC_OK;
}

int ebc_generate_pool(void *handle, const EbcSceneGen *gen, uint32_t seed0, const uint32_t *seeds, int n, int stride) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  GenBatch b;
  if ((rc = generate_batch(h, gen, seed0, seeds, n, b)) != EBC_OK) return rc;
  if ((rc = pool_impl(h, &b.sc, stride, hipMemcpyDeviceToDevice)) != EBC_OK) return rc;
  if (b.poly) return lm_upload(h, nullptr, h->s.E, n, b.poly, b.n_poly, hipMemcpyDeviceToDevice);
  return EBC_OK;
}

int ebc_set_human_actions(void *handle, int location, const double *act) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  if (!act) return fail(EBC_ERR_INVALID, "null actions");
  const size_t bytes = (size_t)h->s.E * h->s.N * 2 * sizeof(double);
  HIP_TRY(hipMemcpyAsync(h->s.hact, act, bytes,
                         location == EBC_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                         h->stream));
  if (location != EBC_DEVICE) HIP_TRY(hipStreamSynchronize(h->stream));
  return EBC_OK;
}

}  // extern "C"

namespace {

// orca_robot_kernel — above 32 rows orca_robot_wide_kernel (ebcsim_orca_wide.hip) — for every env -> d_act [E][2] (device
// pointer), on the handle's stream
int launch_robot_orca(Handle *h, double safety_space, double *d_act) {
  const int others = h->s.N + h->s.S;  // rows of the observation
  if (others > EBC_RO_RW) {  // past the widest lane group: the 10 nearest rows are selected first
    const void *kernel = nullptr;
    int epb = 1;
    ebc_orca_wide_api::robot_kernel(&kernel, &epb);
    void *args[] = {&h->p, &h->s, &safety_space, &d_act, &h->robot_sim};
    HIP_TRY(hipLaunchKernel(kernel, dim3((unsigned)((h->s.E + epb - 1) / epb)), dim3(EBC_WAVE), args, 0, h->stream));
    return EBC_OK;
  }
  const int gs = group_size_for(others);
  const int epw = EBC_WAVE / gs;
  const unsigned blocks = (unsigned)((h->s.E + epw - 1) / epw);
  return with_group_size<kDevRobotGs>(gs, [&](auto g) -> int {
    hipLaunchKernelGGL((ebc::orca_robot_kernel<decltype(g)::value>), dim3(blocks), dim3(EBC_WAVE), 0, h->stream, h->p, h->s, safety_space,
                       d_act, h->robot_sim);
    HIP_TRY(hipGetLastError());
    return EBC_OK;
  });
}

int check_robot_orca(const Handle *h, double safety_space) {
  if (!(safety_space >= 0.0)) return fail(EBC_ERR_INVALID, "safety_space");
  if (h->p.robot_kinematics != EBC_HOLONOMIC) return fail(EBC_ERR_UNSUPPORTED, "ORCA returns ActionXY: holonomic robots only");
  return EBC_OK;  // rows: ebc_create's limit (128), the wide kernel's
}

// The forms whose robot solve is a 32-lane group inside another kernel: the one-launch rollout (EBC_RO_RW) and the
// label kernel of ebc_sail_dagger_k
int check_robot_orca_narrow(const Handle *h, const std::string &who) {
  if (h->s.N + h->s.S > EBC_RO_RW)
    return fail(EBC_ERR_UNSUPPORTED, who + ": robot ORCA: more than 32 observation rows (max_humans + max_static = " +
                                         std::to_string(h->s.N + h->s.S) + ")");
  return EBC_OK;
}

int launch_observe(Handle *h, double *d_ob, float *d_obs) {
  const size_t rows = (size_t)h->s.E * (h->s.N + h->s.S);
  const unsigned blocks = (unsigned)((rows + 255) / 256);
  if (h->T == 17)
    hipLaunchKernelGGL((ebc::observe_kernel<17>), dim3(blocks), dim3(256), 0, h->stream, h->p, h->s, d_ob, d_obs);
  else
    hipLaunchKernelGGL((ebc::observe_kernel<13>), dim3(blocks), dim3(256), 0, h->stream, h->p, h->s, d_ob, d_obs);
  HIP_TRY(hipGetLastError());
  return EBC_OK;
}

size_t om_width(const EbcOmSpec &spec) { return (size_t)spec.cell_num * spec.cell_num * spec.channels; }

// ebc_occupancy_rows' limits on a spec, for this handle's R and T; `what` names the entry in the refusal
int check_om_spec(const Handle *h, const EbcOmSpec *spec, const char *what) {
  const std::string who = std::string(what) + ": ";
  if (spec->channels < 1 || spec->channels > 3)
    return fail(EBC_ERR_UNSUPPORTED, who + "channels not in {1, 2, 3} (" + std::to_string(spec->channels) + ")");
  if (spec->cell_num < 1) return fail(EBC_ERR_UNSUPPORTED, who + "cell_num < 1 (" + std::to_string(spec->cell_num) + ")");
  if (!(std::isfinite(spec->cell_size) && spec->cell_size > 0.0)) return fail(EBC_ERR_UNSUPPORTED, who + "cell_size is not a finite positive number");
  const long long W = (long long)spec->cell_num * spec->cell_num * spec->channels, R = h->s.N + h->s.S;
  if (W > EBC_OM_MAX_WIDTH) return fail(EBC_ERR_UNSUPPORTED, who + "W > 192 map columns (" + std::to_string(W) + ")");
  if (R > EBC_OM_MAX_ROWS) return fail(EBC_ERR_UNSUPPORTED, who + "R > 128 row slots (" + std::to_string(R) + ")");
  if (h->T + W > EBC_OM_MAX_ROW_WIDTH)
    return fail(EBC_ERR_UNSUPPORTED, who + "T + W > 224 columns, the blocks' input limit (" + std::to_string(h->T + W) + ")");
  return EBC_OK;
}

// observe_wide_kernel — `sorted`: observe_wide_sorted_kernel — for every env (a checked spec) -> d_wide [E][R][T + W],
// d_rows [E] or nullptr, on the handle's stream
template <typename Kernel>
int launch_observe_wide_as(Handle *h, Kernel kernel, size_t lds, size_t &raised, const EbcOmSpec &spec, float *d_wide, long long *d_rows) {
  if (lds > 65536 && lds > raised) {  // more than the 64 KB a launch gets by default; a function attribute is per device
    HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    raised = lds;
  }
  const ebc::OmStateSpec sp = {spec.cell_size, spec.cell_num, spec.channels};
  hipLaunchKernelGGL(kernel, dim3((unsigned)h->s.E), dim3(EBC_OMS_THREADS), lds, h->stream, h->p, h->s, sp, d_wide, d_rows);
  HIP_TRY(hipGetLastError());
  return EBC_OK;
}

int launch_observe_wide(Handle *h, const EbcOmSpec &spec, float *d_wide, long long *d_rows, bool sorted = false) {
  if (h->s.E == 0) return EBC_OK;
  const int R = h->s.N + h->s.S, W = (int)om_width(spec);
  static size_t raised_dev[2][2][64] = {{{0}}};
  size_t &raised = raised_dev[sorted][h->T == 17][h->device & 63];
  if (sorted) {
    const size_t lds = ebc::om_state_sorted_lds_bytes(R, W, h->T);  // <= 111 KB at R = 128, W = 192, T = 17
    return h->T == 17 ? launch_observe_wide_as(h, ebc::observe_wide_sorted_kernel<17>, lds, raised, spec, d_wide, d_rows)
                      : launch_observe_wide_as(h, ebc::observe_wide_sorted_kernel<13>, lds, raised, spec, d_wide, d_rows);
  }
  const size_t lds = ebc::om_state_lds_bytes(R, W, h->T);  // <= 110.5 KB at R = 128, W = 192, T = 17
  return h->T == 17 ? launch_observe_wide_as(h, ebc::observe_wide_kernel<17>, lds, raised, spec, d_wide, d_rows)
                    : launch_observe_wide_as(h, ebc::observe_wide_kernel<13>, lds, raised, spec, d_wide, d_rows);
}

// EBC_FLAG_ONE_LAUNCH: rollout_kernel (ebc_rollout.h), a workgroup per group of envs for all K steps.
// EBC_ROBOT_SAIL: the network's LDS area for `chunk` envs, in bytes
unsigned sail_area(const Handle *h, int chunk) { return (unsigned)(ebc::sail_lds_floats(chunk, h->sail_N) * sizeof(float)); }

// ebc_step_k_world: the instantiation that also writes the records (ebcsim_world.hip), with `arg` = the default
// instantiation's argument and the record pointers behind it
template <typename Arg>
int launch_rollout_world(Handle *h, int gs, bool sail, bool mixed, const Arg &arg, const ebc::RolloutWorld &world, unsigned blocks,
                         unsigned lds) {
  ebc::RolloutIOWorld<std::is_same<Arg, ebc::RolloutIOSail>::value> iow;
  static_cast<Arg &>(iow) = arg;
  iow.world = world;
  const void *kernel = nullptr;
  int rc = ebc_world_api::rollout_kernel(gs, sail, mixed, &kernel);
  if (rc != EBC_OK) return rc;
  void *args[] = {&h->p, &h->s, &iow};
  HIP_TRY(hipLaunchKernel(kernel, dim3(blocks), dim3(EBC_RO_THREADS), args, lds, h->stream));
  return EBC_OK;
}

// world: the records of ebc_step_k_world, or nullptr (ebc_step_k)
template <int GS>
int launch_rollout_gs(Handle *h, ebc::RolloutIO io, bool robot_orca, bool mixed, const ebc::RolloutWorld *world) {
  const int N = h->s.N, S = h->s.S, E = h->s.E;
  constexpr unsigned scratch = ebc::RolloutScratch<GS>::BYTES;
  const bool sail = io.robot_policy == EBC_ROBOT_SAIL;
  // envs per workgroup.  Two lower bounds, the larger decides: (1) what gives every wave one pass of ORCA groups per
  // step (the robot's groups take a wave of their own): 2 at 10 humans in 9-lane groups; (2) enough that all workgroups
  // of the launch are resident at once, EBC_RO_OCC per CU — a workgroup stays for K steps, so a second round of
  // workgroups doubles the call: 4 at 4096 envs on 256 CUs, and this is the bound that decides from 2049 envs on.
  // Then the upper bounds: EBC_RO_MAX_EPG, E, and 48 KB of LDS per workgroup.
  int epg = ((robot_orca ? EBC_RO_WAVES - 1 : EBC_RO_WAVES) * (EBC_WAVE / GS)) / N;
  if (!h->cus) {
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
    h->cus = cus > 0 ? cus : 1;
  }
  const int resident = h->cus * EBC_RO_OCC;
  if (epg < (E + resident - 1) / resident) epg = (E + resident - 1) / resident;
  const char *force = getenv("EBCSIM_ONE_LAUNCH_EPG");  // measurements only (environment switches)
  if (force && atoi(force) > 0) epg = atoi(force);
  epg = epg < 1 ? 1 : (epg > EBC_RO_MAX_EPG ? EBC_RO_MAX_EPG : epg);
  epg = epg > E ? E : epg;
  if (sail) {
    // The network's LDS area lies behind the rollout arrays.  One env of each has to fit; then as many envs per
    // workgroup as fit beside a one-env area, then as many envs per pass of the network as fit beside those (at most
    // group_envs, the rows that spread over sail_kernel's waves, and never more than the workgroup has).
    auto bytes = [&](int g, int chunk) { return ebc::rollout_lds(g, N, S, h->T, scratch).bytes + sail_area(h, chunk); };
    if (bytes(1, 1) > 48u * 1024u)
      return fail(EBC_ERR_UNSUPPORTED, "EBC_FLAG_ONE_LAUNCH with EBC_ROBOT_SAIL: one env's rollout arrays (" +
                                           std::to_string(ebc::rollout_lds(1, N, S, h->T, scratch).bytes) +
                                           " bytes) and the network's LDS area for adult_num " + std::to_string(h->sail_N) + " (" +
                                           std::to_string(sail_area(h, 1)) +
                                           " bytes) exceed the kernel's 48 KB of LDS; the per-step form takes this call");
    while (epg > 1 && bytes(epg, 1) > 48u * 1024u) --epg;
    int chunk = ebc_sail::group_envs(h->sail_N);
    chunk = chunk > epg ? epg : chunk;
    while (chunk > 1 && bytes(epg, chunk) > 48u * 1024u) --chunk;
    ebc::RolloutIOSail ios;
    static_cast<ebc::RolloutIO &>(ios) = io;
    ios.epg = epg;
    ios.sail = ebc::RolloutSail{h->sail_P, h->sail_N, chunk};
    if (world) return launch_rollout_world(h, GS, true, mixed, ios, *world, (unsigned)((E + epg - 1) / epg), bytes(epg, chunk));
    if (mixed) {
      const void *kernel = nullptr;
      int rc = ebc_mix_api::rollout_kernel(GS, true, &kernel);
      if (rc != EBC_OK) return rc;
      void *args[] = {&h->p, &h->s, &ios};
      HIP_TRY(hipLaunchKernel(kernel, dim3((unsigned)((E + epg - 1) / epg)), dim3(EBC_RO_THREADS), args, bytes(epg, chunk), h->stream));
      return EBC_OK;
    }
    hipLaunchKernelGGL((ebc::rollout_kernel<GS, true>), dim3((unsigned)((E + epg - 1) / epg)), dim3(EBC_RO_THREADS), bytes(epg, chunk),
                       h->stream, h->p, h->s, ios);
    HIP_TRY(hipGetLastError());
    return EBC_OK;
  }
  while (epg > 1 && ebc::rollout_lds(epg, N, S, h->T, scratch).bytes > 48u * 1024u) --epg;
  const unsigned lds = ebc::rollout_lds(epg, N, S, h->T, scratch).bytes;
  // one env always fits: ebc_create takes at most 33 humans and 128 rows, which is under 30 KB here (the two row
  // buffers are 17 KB of it); the check guards the launch against a later change of those limits
  if (lds > 48u * 1024u) return fail(EBC_ERR_UNSUPPORTED, "EBC_FLAG_ONE_LAUNCH: one env needs more than 48 KB of LDS");
  io.epg = epg;
  const unsigned blocks = (unsigned)((E + epg - 1) / epg);
  if (world) return launch_rollout_world(h, GS, false, mixed, io, *world, blocks, lds);
  if (mixed) {
    const void *kernel = nullptr;
    int rc = ebc_mix_api::rollout_kernel(GS, false, &kernel);
    if (rc != EBC_OK) return rc;
    void *args[] = {&h->p, &h->s, &io};
    HIP_TRY(hipLaunchKernel(kernel, dim3(blocks), dim3(EBC_RO_THREADS), args, lds, h->stream));
    return EBC_OK;
  }
  hipLaunchKernelGGL((ebc::rollout_kernel<GS>), dim3(blocks), dim3(EBC_RO_THREADS), lds, h->stream, h->p, h->s, io);
  HIP_TRY(hipGetLastError());
  return EBC_OK;
}

// mixed: EBC_HUMAN_BY_TYPE (the instantiations of ebcsim_mix.hip)
int launch_rollout(Handle *h, const ebc::RolloutIO &io, bool robot_orca, bool mixed, const ebc::RolloutWorld *world) {
  return with_group_size<kDevHumanGs>(
      h->orca_gs, [&](auto gs) { return launch_rollout_gs<decltype(gs)::value>(h, io, robot_orca, mixed, world); });
}

}  // namespace

extern "C" {

int ebc_robot_orca(void *handle, double safety_space, int location, double *action) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  if (!h->has_reset) return fail(EBC_ERR_STATE, "ebc_robot_orca before ebc_reset");
  if (h->faulted) return fail(EBC_ERR_STATE, "ebc_robot_orca: the handle reported a mailbox fault; ebc_reset re-arms it");
  if (!action) return fail(EBC_ERR_INVALID, "null action");
  if ((rc = check_robot_orca(h, safety_space)) != EBC_OK) return rc;
  double *d_act = action;
  Stager st{h};
  if (location != EBC_DEVICE) {
    if ((rc = ensure_stage(h, pad256((size_t)h->s.E * 2 * 8) + 1024)) != EBC_OK) return rc;
    d_act = st.out(action, (size_t)h->s.E * 2);
  }
  if ((rc = launch_robot_orca(h, safety_space, d_act)) != EBC_OK) return rc;
  if (location != EBC_DEVICE) return st.finish();
  return EBC_OK;
}

int ebc_set_human_policies(void *handle, const int32_t policy_of_type[3]) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  if (!policy_of_type) return fail(EBC_ERR_INVALID, "ebc_set_human_policies: policy_of_type is NULL");
  static const char *const kType[3] = {"EBC_ADULT", "EBC_BICYCLE", "EBC_CHILD"};
  unsigned linear = 0;
  for (int t = 0; t < 3; ++t) {
    if (policy_of_type[t] != EBC_HUMAN_ORCA && policy_of_type[t] != EBC_HUMAN_LINEAR)
      return fail(EBC_ERR_INVALID, std::string("ebc_set_human_policies: policy_of_type[") + kType[t] + "] = " +
                                       std::to_string(policy_of_type[t]) + " (EBC_HUMAN_ORCA or EBC_HUMAN_LINEAR)");
    if (policy_of_type[t] == EBC_HUMAN_LINEAR) linear |= 1u << t;
  }
  h->s.human_linear = linear;  // travels with every launch from now on (DevState is a kernel argument)
  return EBC_OK;
}

int ebc_robot_sail(void *handle, void *sail) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  if (!sail) {
    if (h->sail_P) HIP_TRY(hipStreamSynchronize(h->stream));  // nothing enqueued still reads the weights being detached
    h->sail_P = nullptr;
    h->sail_N = 0;
    return EBC_OK;
  }
  const ebc_sail_api::View v = ebc_sail_api::view(sail);
  if (v.P == h->sail_P && v.N == h->sail_N) return EBC_OK;  // attached already
  if (v.device != h->device)
    return fail(EBC_ERR_INVALID, "ebc_robot_sail: the network is on device " + std::to_string(v.device) + ", the env handle on device " +
                                     std::to_string(h->device));
  if (h->s.N + h->s.S < v.N)
    return fail(EBC_ERR_INVALID, "ebc_robot_sail: the env has " + std::to_string(h->s.N + h->s.S) +
                                     " observation rows (max_humans + max_static), the network takes exactly adult_num = " + std::to_string(v.N));
  if (h->sail_P) HIP_TRY(hipStreamSynchronize(h->stream));  // as for a detach: another network takes its place
  h->sail_P = v.P;
  h->sail_N = v.N;
  return EBC_OK;
}

int ebc_robot_orca_sim(void *handle, int enable) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  const size_t E = h->s.E, R = (size_t)h->s.N + h->s.S;
  if (!enable) {  // the arrays stay allocated (freed with the handle); the kernels get no simulator
    h->robot_sim.rows = nullptr;
    return EBC_OK;
  }
  if (!h->robot_sim.radius) {
    int *rows = nullptr;
    if ((rc = dev_alloc(h, &rows, E)) != EBC_OK) return rc;
    if ((rc = dev_alloc(h, &h->robot_sim.radius, E * R)) != EBC_OK) return rc;
    if ((rc = dev_alloc(h, &h->robot_sim.self, E)) != EBC_OK) return rc;
    h->robot_sim_rows = rows;
  }
  h->robot_sim.rows = h->robot_sim_rows;
  HIP_TRY(hipMemset(h->robot_sim.rows, 0xff, E * sizeof(int)));  // -1: no simulator yet (a fresh policy object)
  return EBC_OK;
}

int ebc_robot_orca_sim_state(void *handle, int location, int set, int32_t *rows, float *radius, float *self) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  if (!h->robot_sim.rows) return fail(EBC_ERR_STATE, "ebc_robot_orca_sim_state: no persistent simulator (ebc_robot_orca_sim)");
  if (!rows || !radius || !self) return fail(EBC_ERR_INVALID, "null argument");
  const size_t E = h->s.E, R = (size_t)h->s.N + h->s.S;
  HIP_TRY(hipStreamSynchronize(h->stream));
  const hipMemcpyKind kind = location == EBC_DEVICE ? hipMemcpyDeviceToDevice : (set ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost);
  if (set) {
    HIP_TRY(hipMemcpy(h->robot_sim.rows, rows, E * sizeof(int), kind));
    HIP_TRY(hipMemcpy(h->robot_sim.radius, radius, E * R * sizeof(float), kind));
    HIP_TRY(hipMemcpy(h->robot_sim.self, self, E * 2 * sizeof(float), kind));
  } else {
    HIP_TRY(hipMemcpy(rows, h->robot_sim.rows, E * sizeof(int), kind));
    HIP_TRY(hipMemcpy(radius, h->robot_sim.radius, E * R * sizeof(float), kind));
    HIP_TRY(hipMemcpy(self, h->robot_sim.self, E * 2 * sizeof(float), kind));
  }
  return EBC_OK;
}

// A step's launch carries per-call state (the double-buffered robot, the launch counter of the mailboxes): replayed
// from a HIP graph it would run with the arguments of the capture.  Refused where it would be recorded.
static int refuse_capture(Handle *h, const char *what) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(h->stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone)
    return fail(EBC_ERR_UNSUPPORTED, std::string(what) + ": the stream is being captured into a HIP graph; a step must be launched, not replayed");
  return EBC_OK;
}

// ebc_step_k; with `om` (ebc_step_k_om) the wide state of every state the policy sees, enqueued before step k; with
// `world` (ebc_step_k_world) the robot's FullState and the world-frame rows before step k
static int step_k_impl(void *handle, const EbcStepKArgs *a, const EbcStepKOm *om, const EbcStepKWorld *world, const char *what) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  const std::string who = what;
  if (!a || a->struct_size != sizeof(EbcStepKArgs)) return fail(EBC_ERR_INVALID, "EbcStepKArgs.struct_size");
  if (!h->has_reset) return fail(EBC_ERR_STATE, who + " before ebc_reset");
  if (h->faulted) return fail(EBC_ERR_STATE, who + ": the handle reported a mailbox fault; ebc_reset re-arms it");
  if ((rc = refuse_capture(h, what)) != EBC_OK) return rc;
  if (om) {
    if (!om->state_wide) return fail(EBC_ERR_INVALID, who + ": state_wide is NULL");
    if ((rc = check_om_spec(h, &om->spec, what)) != EBC_OK) return rc;
    if (a->flags & EBC_FLAG_ONE_LAUNCH)
      return fail(EBC_ERR_UNSUPPORTED, who + ": EBC_FLAG_ONE_LAUNCH (the window with maps has the per-step form only)");
  }
  if (a->K < 1) return fail(EBC_ERR_INVALID, "K");
  if (a->human_policy != EBC_HUMAN_ORCA && a->human_policy != EBC_HUMAN_LINEAR && a->human_policy != EBC_HUMAN_EXTERNAL &&
      a->human_policy != EBC_HUMAN_BY_TYPE)
    return fail(EBC_ERR_INVALID, "human_policy (a cached look-ahead holds for one step only)");
  if (a->robot_policy != EBC_ROBOT_EXTERNAL && a->robot_policy != EBC_ROBOT_LINEAR && a->robot_policy != EBC_ROBOT_ORCA &&
      a->robot_policy != EBC_ROBOT_SAIL)
    return fail(EBC_ERR_INVALID, "robot_policy");
  const bool sail = a->robot_policy == EBC_ROBOT_SAIL;
  if (sail && !h->sail_P) return fail(EBC_ERR_STATE, who + ": EBC_ROBOT_SAIL with no network attached (ebc_robot_sail)");
  if (a->robot_policy == EBC_ROBOT_EXTERNAL && !a->robot_action) return fail(EBC_ERR_INVALID, "robot_action is NULL");
  if (a->robot_policy == EBC_ROBOT_LINEAR && h->p.robot_kinematics != EBC_HOLONOMIC)
    return fail(EBC_ERR_UNSUPPORTED, "the linear robot policy is holonomic (simulator/policy/linear.py:11)");
  if (a->robot_policy == EBC_ROBOT_ORCA && (rc = check_robot_orca(h, a->robot_safety_space)) != EBC_OK) return rc;
  if (a->flags & EBC_FLAG_BORDER) return fail(EBC_ERR_UNSUPPORTED, who + ": no border");
  const bool one_launch = (a->flags & EBC_FLAG_ONE_LAUNCH) != 0;
  // strict: a caller who sets the flag knows which form ran
  if (one_launch && a->human_policy == EBC_HUMAN_LINEAR)
    return fail(EBC_ERR_UNSUPPORTED, who + ": EBC_FLAG_ONE_LAUNCH with EBC_HUMAN_LINEAR (the one-launch form moves ORCA humans only)");
  if (one_launch && a->human_policy == EBC_HUMAN_EXTERNAL)
    return fail(EBC_ERR_UNSUPPORTED, who + ": EBC_FLAG_ONE_LAUNCH with EBC_HUMAN_EXTERNAL (the one-launch form moves ORCA humans only)");
  if (one_launch && a->robot_policy == EBC_ROBOT_ORCA && (rc = check_robot_orca_narrow(h, who + ": EBC_FLAG_ONE_LAUNCH")) != EBC_OK)
    return rc;
  const DevState &s = h->s;
  const size_t E = s.E, R = s.N + s.S, T = h->T, K = (size_t)a->K;
  const double *d_act_in = a->robot_action;
  float *d_state = a->state_rotated, *d_obs = a->obs_rotated;
  long long *d_rows = a->n_rows;
  double *d_act_out = a->robot_action_out, *d_reward = a->reward, *d_dmin = a->dmin, *d_goal = a->dist_to_goal;
  uint8_t *d_done = a->done, *d_info = a->info;
  double *d_wrobot = world ? world->robot : nullptr, *d_wob = world ? world->ob : nullptr;
  Stager st{h};
  if (a->location != EBC_DEVICE) {
    const size_t need = K * (pad256(E * 2 * 8) * 2 + pad256(E * 8) * 3 + pad256(E) * 2 + pad256(E * 3 * 8) +
                             pad256(E * R * T * 4) * 2) + pad256(E * 2 * 8) + 8192 +
                        (world ? pad256(K * E * 9 * 8) + pad256(K * E * R * 5 * 8) : 0);
    if ((rc = ensure_stage(h, need)) != EBC_OK) return rc;
    if ((rc = st.in(a->robot_policy == EBC_ROBOT_EXTERNAL ? a->robot_action : nullptr, K * E * 2, &d_act_in)) != EBC_OK) return rc;
    d_state = st.out(a->state_rotated, K * E * R * T); d_rows = st.out(a->n_rows, K * E);
    d_act_out = st.out(a->robot_action_out, K * E * 2); d_reward = st.out(a->reward, K * E);
    d_done = st.out(a->done, K * E); d_info = st.out(a->info, K * E); d_dmin = st.out(a->dmin, K * E * 3);
    d_goal = st.out(a->dist_to_goal, K * E); d_obs = st.out(a->obs_rotated, K * E * R * T);
    d_wrobot = st.out(d_wrobot, K * E * 9); d_wob = st.out(d_wob, K * E * R * 5);
  }
  if (one_launch) {
    ebc::RolloutIO io;
    memset(&io, 0, sizeof(io));
    io.K = a->K;
    io.robot_policy = a->robot_policy;
    io.auto_reset = (a->flags & EBC_FLAG_AUTO_RESET) ? 1 : 0;
    io.T = h->T;
    io.safety_space = a->robot_safety_space;
    if (a->robot_policy == EBC_ROBOT_ORCA) io.sim = h->robot_sim;
    io.robot_action = a->robot_policy == EBC_ROBOT_EXTERNAL ? d_act_in : nullptr;
    io.state_rotated = d_state; io.n_rows = d_rows; io.robot_action_out = d_act_out; io.reward = d_reward;
    io.done = d_done; io.info = d_info; io.dmin = d_dmin; io.dist_to_goal = d_goal; io.obs_rotated = d_obs;
    const ebc::RolloutWorld records = {d_wrobot, d_wob};
    if ((rc = launch_rollout(h, io, a->robot_policy == EBC_ROBOT_ORCA, a->human_policy == EBC_HUMAN_BY_TYPE, world ? &records : nullptr)) !=
        EBC_OK)
      return rc;
    if (a->location != EBC_DEVICE) return st.finish();
    return EBC_OK;
  }
  if (sail && !h->sail_rows) {  // the gathers the network reads (DeviceSailPolicy's buffers)
    if ((rc = dev_alloc(h, &h->sail_robot, E * 9)) != EBC_OK) return rc;
    if ((rc = dev_alloc(h, &h->sail_ob, E * R * 5)) != EBC_OK) return rc;
    if ((rc = dev_alloc(h, &h->sail_rows, E)) != EBC_OK) return rc;
  }
  // the ORCA or SAIL robot's action of step k needs a home when the caller does not ask for the actions
  double *orca_act = nullptr;
  if ((a->robot_policy == EBC_ROBOT_ORCA || sail) && !d_act_out) {
    if (a->location != EBC_DEVICE) {
      orca_act = (double *)((char *)h->stage + st.off);
      st.off += pad256(E * 2 * 8);
    } else {
      if (!h->act_scratch) {
        void *ptr = nullptr;
        HIP_TRY(hipMalloc(&ptr, E * 2 * 8));
        h->allocs.push_back(ptr);
        h->act_scratch = (double *)ptr;
      }
      orca_act = h->act_scratch;
    }
  }
  for (size_t k = 0; k < K; ++k) {
    if (om && (rc = launch_observe_wide(h, om->spec, om->state_wide + k * E * R * (T + om_width(om->spec)), nullptr)) != EBC_OK) return rc;
    if (d_wrobot) HIP_TRY(hipMemcpyAsync(d_wrobot + k * E * 9, h->s.robot, E * 9 * 8, hipMemcpyDeviceToDevice, h->stream));
    // one launch of observe_kernel for the rotated state and the world-frame rows, whichever are asked for
    if ((d_state || d_wob) &&
        (rc = launch_observe(h, d_wob ? d_wob + k * E * R * 5 : nullptr, d_state ? d_state + k * E * R * T : nullptr)) != EBC_OK)
      return rc;
    if (d_rows) {
      hipLaunchKernelGGL(ebc::row_counts_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, h->stream, h->s, d_rows + k * E);
      HIP_TRY(hipGetLastError());
    }
    StepIO io;
    memset(&io, 0, sizeof(io));
    io.auto_reset = (a->flags & EBC_FLAG_AUTO_RESET) ? 1 : 0;
    io.robot_policy = a->robot_policy == EBC_ROBOT_LINEAR ? EBC_ROBOT_LINEAR : EBC_ROBOT_EXTERNAL;
    if (a->robot_policy == EBC_ROBOT_ORCA) {
      double *act = d_act_out ? d_act_out + k * E * 2 : orca_act;
      if ((rc = launch_robot_orca(h, a->robot_safety_space, act)) != EBC_OK) return rc;
      io.robot_action = act;
    } else if (sail) {  // DeviceSailPolicy.decide: ebc_get_state's robot, ebc_observe's ob, ebc_row_counts, sail_kernel
      double *act = d_act_out ? d_act_out + k * E * 2 : orca_act;
      HIP_TRY(hipMemcpyAsync(h->sail_robot, h->s.robot, E * 9 * 8, hipMemcpyDeviceToDevice, h->stream));
      if ((rc = launch_observe(h, h->sail_ob, nullptr)) != EBC_OK) return rc;
      hipLaunchKernelGGL(ebc::row_counts_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, h->stream, h->s, h->sail_rows);
      HIP_TRY(hipGetLastError());
      if ((rc = ebc_sail_api::launch(h->sail_P, h->sail_N, h->stream, h->sail_robot, h->sail_ob, h->sail_rows, act, nullptr, (int)E,
                                     (int)R)) != EBC_OK)
        return rc;
      io.robot_action = act;
    } else if (a->robot_policy == EBC_ROBOT_EXTERNAL) {
      io.robot_action = d_act_in + k * E * 2;
    }
    io.reward = d_reward ? d_reward + k * E : nullptr;
    io.done = d_done ? d_done + k * E : nullptr;
    io.info = d_info ? d_info + k * E : nullptr;
    io.dmin = d_dmin ? d_dmin + k * E * 3 : nullptr;
    io.dist_to_goal = d_goal ? d_goal + k * E : nullptr;
    // with EBC_ROBOT_ORCA and _SAIL the step reads the action from where the policy left it (already robot_action_out[k])
    io.robot_action_out = (a->robot_policy != EBC_ROBOT_ORCA && !sail && d_act_out) ? d_act_out + k * E * 2 : nullptr;
    io.obs_rotated = d_obs ? d_obs + k * E * R * T : nullptr;
    if ((rc = launch_step(h, io, a->human_policy)) != EBC_OK) return rc;
  }
  if (a->location != EBC_DEVICE) return st.finish();
  return EBC_OK;
}

int ebc_step_k(void *handle, const EbcStepKArgs *a) { return step_k_impl(handle, a, nullptr, nullptr, "ebc_step_k"); }

int ebc_step_k_om(void *handle, const EbcStepKArgs *a, const EbcStepKOm *om) {
  if (!om) return fail(EBC_ERR_INVALID, "ebc_step_k_om: om is NULL");
  if (om->struct_size != sizeof(EbcStepKOm)) return fail(EBC_ERR_INVALID, "EbcStepKOm.struct_size");
  if (om->spec.struct_size != sizeof(EbcOmSpec)) return fail(EBC_ERR_INVALID, "EbcOmSpec.struct_size");
  return step_k_impl(handle, a, om, nullptr, "ebc_step_k_om");
}

int ebc_step_k_world(void *handle, const EbcStepKArgs *a, const EbcStepKWorld *world) {
  if (!world) return fail(EBC_ERR_INVALID, "ebc_step_k_world: world is NULL");
  if (world->struct_size != sizeof(EbcStepKWorld)) return fail(EBC_ERR_INVALID, "EbcStepKWorld.struct_size");
  if (world->reserved != 0) return fail(EBC_ERR_INVALID, "EbcStepKWorld.reserved");
  if (!world->robot && !world->ob) return fail(EBC_ERR_INVALID, "ebc_step_k_world: robot and ob are both NULL");
  return step_k_impl(handle, a, nullptr, world, "ebc_step_k_world");
}

// K closed-loop steps of the attached SAIL network with the ORCA robot labelling every state (csrc/ebc_dagger.h): per
// step the label kernel, the network, the select and the step, four launches.
int ebc_sail_dagger_k(void *handle, const EbcSailDaggerArgs *a) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  if (!a || a->struct_size != sizeof(EbcSailDaggerArgs)) return fail(EBC_ERR_INVALID, "EbcSailDaggerArgs.struct_size");
  if (!h->has_reset) return fail(EBC_ERR_STATE, "ebc_sail_dagger_k before ebc_reset");
  if (h->faulted) return fail(EBC_ERR_STATE, "ebc_sail_dagger_k: the handle reported a mailbox fault; ebc_reset re-arms it");
  if ((rc = refuse_capture(h, "ebc_sail_dagger_k")) != EBC_OK) return rc;
  if (a->K < 1) return fail(EBC_ERR_INVALID, "K");
  if (a->human_policy != EBC_HUMAN_ORCA && a->human_policy != EBC_HUMAN_LINEAR && a->human_policy != EBC_HUMAN_EXTERNAL &&
      a->human_policy != EBC_HUMAN_BY_TYPE)
    return fail(EBC_ERR_INVALID, "human_policy (a cached look-ahead holds for one step only)");
  if (!h->sail_P) return fail(EBC_ERR_STATE, "ebc_sail_dagger_k: no network attached (ebc_robot_sail)");
  if ((rc = check_robot_orca(h, a->expert_safety_space)) != EBC_OK) return rc;
  if ((rc = check_robot_orca_narrow(h, "ebc_sail_dagger_k")) != EBC_OK) return rc;
  if (a->flags & EBC_FLAG_BORDER) return fail(EBC_ERR_UNSUPPORTED, "ebc_sail_dagger_k: no border");
  if (a->flags & EBC_FLAG_ONE_LAUNCH)
    return fail(EBC_ERR_UNSUPPORTED, "ebc_sail_dagger_k: EBC_FLAG_ONE_LAUNCH (the labelled rollout has the per-step form only)");
  if (a->flags & ~EBC_FLAG_AUTO_RESET) return fail(EBC_ERR_INVALID, "flags");
  if (!a->robot || !a->ob || !a->n_rows || !a->learner_action || !a->expert_action || !a->robot_action_out)
    return fail(EBC_ERR_INVALID, "ebc_sail_dagger_k: a required output is NULL (robot, ob, n_rows, learner_action, expert_action, robot_action_out)");
  const size_t E = h->s.E, R = h->s.N + h->s.S, K = (size_t)a->K;
  const int gs = group_size_for((int)R);
  const int epw = EBC_WAVE / gs;
  const unsigned label_blocks = (unsigned)((E + epw - 1) / epw);
  const unsigned select_blocks = (unsigned)((2 * E + 255) / 256);
  for (size_t k = 0; k < K; ++k) {
    double *robot = a->robot + k * E * 9, *ob = a->ob + k * E * R * 5;
    long long *rows = a->n_rows + k * E;
    double *learner = a->learner_action + k * E * 2, *expert = a->expert_action + k * E * 2, *act = a->robot_action_out + k * E * 2;
    rc = with_group_size<kDevRobotGs>(gs, [&](auto g) -> int {
      hipLaunchKernelGGL((ebc::dagger_label_kernel<decltype(g)::value>), dim3(label_blocks), dim3(EBC_WAVE), 0, h->stream, h->p, h->s,
                         a->expert_safety_space, h->robot_sim, robot, ob, rows, expert);
      HIP_TRY(hipGetLastError());
      return EBC_OK;
    });
    if (rc != EBC_OK) return rc;
    // the network reads the step's records where the label kernel left them
    if ((rc = ebc_sail_api::launch(h->sail_P, h->sail_N, h->stream, robot, ob, rows, learner, nullptr, (int)E, (int)R)) != EBC_OK) return rc;
    hipLaunchKernelGGL(ebc::dagger_select_kernel, dim3(select_blocks), dim3(256), 0, h->stream, (int)E,
                       a->take_expert ? a->take_expert + k * E : nullptr, reinterpret_cast<const unsigned long long *>(learner),
                       reinterpret_cast<const unsigned long long *>(expert), reinterpret_cast<unsigned long long *>(act));
    HIP_TRY(hipGetLastError());
    StepIO io;
    memset(&io, 0, sizeof(io));
    io.auto_reset = (a->flags & EBC_FLAG_AUTO_RESET) ? 1 : 0;
    io.robot_policy = EBC_ROBOT_EXTERNAL;
    io.robot_action = act;
    io.reward = a->reward ? a->reward + k * E : nullptr;
    io.done = a->done ? a->done + k * E : nullptr;
    io.info = a->info ? a->info + k * E : nullptr;
    if ((rc = launch_step(h, io, a->human_policy)) != EBC_OK) return rc;
  }
  return EBC_OK;
}

// ebc_step, and with `local_map` (ebc_step_with_map) the map of every env's post-step state, enqueued first
static int step_impl(Handle *h, const EbcStepArgs *a, double *local_map, const char *what) {
  int rc;
  if (!a || a->struct_size != sizeof(EbcStepArgs)) return fail(EBC_ERR_INVALID, "EbcStepArgs.struct_size");
  if (!h->has_reset) return fail(EBC_ERR_STATE, std::string(what) + " before ebc_reset");
  if (h->faulted) return fail(EBC_ERR_STATE, std::string(what) + ": the handle reported a mailbox fault; ebc_reset re-arms it");
  if ((rc = refuse_capture(h, what)) != EBC_OK) return rc;
  if (a->human_policy < EBC_HUMAN_EXTERNAL || a->human_policy > EBC_HUMAN_BY_TYPE)
    return fail(EBC_ERR_INVALID, "human_policy");
  if (a->robot_policy == EBC_ROBOT_LINEAR && h->p.robot_kinematics != EBC_HOLONOMIC)
    return fail(EBC_ERR_UNSUPPORTED, "the linear robot policy is holonomic (simulator/policy/linear.py:11)");
  if (a->robot_policy == EBC_ROBOT_EXTERNAL && !a->robot_action)
    return fail(EBC_ERR_INVALID, "robot_action is NULL");
  if (a->robot_policy != EBC_ROBOT_EXTERNAL && a->robot_policy != EBC_ROBOT_LINEAR)
    return fail(EBC_ERR_INVALID, "robot_policy");
  if ((a->flags & EBC_FLAG_BORDER) && !a->border) return fail(EBC_ERR_INVALID, "border is NULL");
  if (local_map && (rc = lm_ready(h, what)) != EBC_OK) return rc;
  const DevState &s = h->s;
  const size_t E = s.E, N = s.N, R = s.N + s.S, T = h->T;
  double *d_map = local_map;
  StepIO io;
  memset(&io, 0, sizeof(io));
  io.robot_policy = a->robot_policy;
  io.auto_reset = (a->flags & EBC_FLAG_AUTO_RESET) ? 1 : 0;
  io.has_border = (a->flags & EBC_FLAG_BORDER) ? 1 : 0;
  if (io.has_border) memcpy(io.border, a->border, sizeof(io.border));
  Stager st{h};
  if (a->location == EBC_DEVICE) {
    io.robot_action = a->robot_action;
    io.reward = a->reward; io.done = a->done; io.info = a->info; io.dmin = a->dmin;
    io.dist_to_goal = a->dist_to_goal; io.robot_action_out = a->robot_action_out;
    io.human_action = a->human_action; io.ob = a->ob; io.obs_rotated = a->obs_rotated;
  } else {
    const size_t need = pad256(E * 2 * 8) * 2 + pad256(E * 8) * 2 + pad256(E) * 2 + pad256(E * 3 * 8) +
                        pad256(E * N * 2 * 8) + pad256(E * R * 5 * 8) + pad256(E * R * T * 4) + 4096 +
                        (local_map ? pad256(E * h->lm.dim * 8) : 0);
    if ((rc = ensure_stage(h, need)) != EBC_OK) return rc;
    if ((rc = st.in(a->robot_policy == EBC_ROBOT_EXTERNAL ? a->robot_action : nullptr, E * 2,
                    &io.robot_action)) != EBC_OK)
      return rc;
    io.reward = st.out(a->reward, E); io.done = st.out(a->done, E); io.info = st.out(a->info, E);
    io.dmin = st.out(a->dmin, E * 3); io.dist_to_goal = st.out(a->dist_to_goal, E);
    io.robot_action_out = st.out(a->robot_action_out, E * 2);
    io.human_action = st.out(a->human_action, E * N * 2); io.ob = st.out(a->ob, E * R * 5);
    io.obs_rotated = st.out(a->obs_rotated, E * R * T);
    d_map = st.out(local_map, E * h->lm.dim);
  }
  // the map reads the pre-step state (and the slot it runs, before a restart rewrites it): launched first
  if (d_map && (rc = launch_local_map(h, 1, io.robot_policy, io.robot_action, d_map)) != EBC_OK) return rc;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (h->timing) {
    if (h->ev_used + 2 > h->ev.size()) {
      for (int q = 0; q < 2; ++q) {
        hipEvent_t ev;
        HIP_TRY(hipEventCreate(&ev));
        h->ev.push_back(ev);
      }
    }
    e0 = h->ev[h->ev_used++];
    e1 = h->ev[h->ev_used++];
    HIP_TRY(hipEventRecord(e0, h->stream));
  }
  if ((rc = launch_step(h, io, a->human_policy)) != EBC_OK) return rc;
  if (h->timing) HIP_TRY(hipEventRecord(e1, h->stream));
  if (a->location != EBC_DEVICE) return st.finish();
  return EBC_OK;
}

int ebc_step(void *handle, const EbcStepArgs *a) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  return step_impl(h, a, nullptr, "ebc_step");
}

int ebc_step_with_map(void *handle, const EbcStepArgs *a, double *local_map) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  if (!local_map) return fail(EBC_ERR_INVALID, "ebc_step_with_map: local_map is NULL");
  return step_impl(h, a, local_map, "ebc_step_with_map");
}

int ebc_local_map_config(void *handle, const EbcLocalMapParams *lp) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  if (!lp || lp->struct_size != sizeof(EbcLocalMapParams)) return fail(EBC_ERR_INVALID, "EbcLocalMapParams.struct_size");
  if (lp->dim <= 0) return fail(EBC_ERR_INVALID, "local map dim");
  if (lp->dim > EBC_LM_MAX_DIM) return fail(EBC_ERR_UNSUPPORTED, "local map dim > 128");
  if (!(lp->max_range > 0) || !std::isfinite(lp->max_range)) return fail(EBC_ERR_INVALID, "local map max_range");
  if (!(lp->angle_max > lp->angle_min) || !std::isfinite(lp->angle_min) || !std::isfinite(lp->angle_max))
    return fail(EBC_ERR_INVALID, "local map angle_min / angle_max");
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (!h->lm_on) {
    if ((rc = lm_alloc(h, h->s.E + h->s.pool.P, 0)) != EBC_OK) return rc;
    h->lm_on = true;
  }
  h->lm = ebc::local_map_cfg(lp->dim, lp->max_range, lp->angle_min, lp->angle_max, lp->normalize ? 1 : 0);
  return EBC_OK;
}

}  // extern "C"

namespace {
// The polygons of n scenes: rectangles with axis-aligned sides (the generator's and every saved scene's), <= S of them.
int validate_obstacles(const Handle *h, const EbcObstacles *o) {
  if (!o || o->struct_size != sizeof(EbcObstacles)) return fail(EBC_ERR_INVALID, "EbcObstacles.struct_size");
  if (o->n <= 0 || !o->n_poly || !o->vertices) return fail(EBC_ERR_INVALID, "EbcObstacles: n, n_poly, vertices");
  const size_t S1 = lm_s1(h);
  for (int r = 0; r < o->n; ++r) {
    if (o->n_poly[r] < 0 || o->n_poly[r] > h->s.S)
      return fail(EBC_ERR_INVALID, "EbcObstacles: scene " + std::to_string(r) + " has more than max_static polygons");
    for (int q = 0; q < o->n_poly[r]; ++q) {
      const double *v = o->vertices + ((size_t)r * S1 + q) * 8;
      bool finite = true;
      for (int k = 0; k < 8; ++k) finite = finite && std::isfinite(v[k]);
      // v0 -> v1 -> v2 -> v3: sides alternately horizontal and vertical, in either order, none of length 0
      const bool hv = v[1] == v[3] && v[2] == v[4] && v[5] == v[7] && v[6] == v[0];
      const bool vh = v[0] == v[2] && v[3] == v[5] && v[4] == v[6] && v[7] == v[1];
      const bool open = v[0] != v[4] && v[1] != v[5];
      if (!finite || !(hv || vh) || !open)
        return fail(EBC_ERR_INVALID, "EbcObstacles: polygon " + std::to_string(q) + " of scene " + std::to_string(r) +
                                         " is not an axis-aligned 4-vertex rectangle");
    }
  }
  return EBC_OK;
}
}  // namespace

extern "C" {

int ebc_set_obstacles(void *handle, const int32_t *env_ids, const EbcObstacles *o) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  if (!h->lm_on) return fail(EBC_ERR_STATE, "ebc_set_obstacles before ebc_local_map_config");
  if ((rc = validate_obstacles(h, o)) != EBC_OK) return rc;
  if (o->n > h->s.E) return fail(EBC_ERR_INVALID, "EbcObstacles.n > n_envs");
  for (int r = 0; env_ids && r < o->n; ++r)
    if (env_ids[r] < 0 || env_ids[r] >= h->s.E) return fail(EBC_ERR_INVALID, "env id out of range");
  HIP_TRY(hipStreamSynchronize(h->stream));
  return lm_upload(h, env_ids, 0, o->n, o->vertices, o->n_poly, hipMemcpyHostToDevice);
}

int ebc_set_obstacle_pool(void *handle, const EbcObstacles *o) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  if (!h->lm_on) return fail(EBC_ERR_STATE, "ebc_set_obstacle_pool before ebc_local_map_config");
  if ((rc = validate_obstacles(h, o)) != EBC_OK) return rc;
  if (h->s.pool.P == 0 || o->n != h->s.pool.P)
    return fail(EBC_ERR_INVALID, "ebc_set_obstacle_pool: n must equal the installed pool's size");
  HIP_TRY(hipStreamSynchronize(h->stream));
  return lm_upload(h, nullptr, h->s.E, o->n, o->vertices, o->n_poly, hipMemcpyHostToDevice);
}

int ebc_local_map(void *handle, int location, double *out) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  if (!out) return fail(EBC_ERR_INVALID, "ebc_local_map: out is NULL");
  if (!h->has_reset) return fail(EBC_ERR_STATE, "ebc_local_map before ebc_reset");
  if (h->faulted) return fail(EBC_ERR_STATE, "ebc_local_map: the handle reported a mailbox fault; ebc_reset re-arms it");
  if ((rc = lm_ready(h, "ebc_local_map")) != EBC_OK) return rc;
  double *d_out = out;
  Stager st{h};
  if (location != EBC_DEVICE) {
    if ((rc = ensure_stage(h, pad256((size_t)h->s.E * h->lm.dim * 8) + 1024)) != EBC_OK) return rc;
    d_out = st.out(out, (size_t)h->s.E * h->lm.dim);
  }
  if ((rc = launch_local_map(h, 0, EBC_ROBOT_EXTERNAL, nullptr, d_out)) != EBC_OK) return rc;
  if (location != EBC_DEVICE) return st.finish();
  return EBC_OK;
}

int ebc_observe(void *handle, int location, double *ob, float *obs_rotated) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  if (!h->has_reset) return fail(EBC_ERR_STATE, "ebc_observe before ebc_reset");
  if (h->faulted) return fail(EBC_ERR_STATE, "ebc_observe: the handle reported a mailbox fault; ebc_reset re-arms it");
  const DevState &s = h->s;
  const size_t rows = (size_t)s.E * (s.N + s.S), T = h->T;
  double *d_ob = ob;
  float *d_obs = obs_rotated;
  Stager st{h};
  if (location != EBC_DEVICE) {
    if ((rc = ensure_stage(h, pad256(rows * 5 * 8) + pad256(rows * T * 4) + 1024)) != EBC_OK) return rc;
    d_ob = st.out(ob, rows * 5);
    d_obs = st.out(obs_rotated, rows * T);
  }
  if ((rc = launch_observe(h, d_ob, d_obs)) != EBC_OK) return rc;
  if (location != EBC_DEVICE) return st.finish();
  return EBC_OK;
}

int ebc_lookahead(void *handle, const EbcLookaheadArgs *a) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  if (!a || a->struct_size != sizeof(EbcLookaheadArgs))
    return fail(EBC_ERR_INVALID, "EbcLookaheadArgs.struct_size");
  if (!h->has_reset) return fail(EBC_ERR_STATE, "ebc_lookahead before ebc_reset");
  if (h->faulted) return fail(EBC_ERR_STATE, "ebc_lookahead: the handle reported a mailbox fault; ebc_reset re-arms it");
  if (!a->actions || a->n_actions <= 0) return fail(EBC_ERR_INVALID, "actions");
  if (a->n_actions > EBC_LA_MAX_ACTIONS) return fail(EBC_ERR_UNSUPPORTED, "more than 128 actions");
  if (a->human_policy != EBC_HUMAN_ORCA && a->human_policy != EBC_HUMAN_LINEAR &&
      a->human_policy != EBC_HUMAN_EXTERNAL && a->human_policy != EBC_HUMAN_CACHED && a->human_policy != EBC_HUMAN_BY_TYPE)
    return fail(EBC_ERR_INVALID, "human_policy");
  if ((a->flags & EBC_FLAG_BORDER) && !a->border) return fail(EBC_ERR_INVALID, "border is NULL");
  const DevState &s = h->s;
  const size_t E = s.E, R = s.N + s.S, T = h->T, A = a->n_actions;
  LookIO io;
  memset(&io, 0, sizeof(io));
  io.A = a->n_actions;
  io.has_border = (a->flags & EBC_FLAG_BORDER) ? 1 : 0;
  if (io.has_border) memcpy(io.border, a->border, sizeof(io.border));
  Stager st{h};
  if (a->location == EBC_DEVICE) {
    io.actions = a->actions;
    io.reward = a->reward; io.done = a->done; io.info = a->info; io.dmin = a->dmin;
    io.next_ob = a->next_ob; io.rows = a->rows_rotated;
  } else {
    const size_t need = pad256(A * 2 * 8) + pad256(E * A * 8) + pad256(E * A) * 2 + pad256(E * A * 3 * 8) +
                        pad256(E * R * 5 * 8) + (a->rows_rotated ? pad256(E * A * R * T * 4) : 0) + 4096;
    if ((rc = ensure_stage(h, need)) != EBC_OK) return rc;
    if ((rc = st.in(a->actions, A * 2, &io.actions)) != EBC_OK) return rc;
    io.reward = st.out(a->reward, E * A); io.done = st.out(a->done, E * A);
    io.info = st.out(a->info, E * A); io.dmin = st.out(a->dmin, E * A * 3);
    io.next_ob = st.out(a->next_ob, E * R * 5); io.rows = st.out(a->rows_rotated, E * A * R * T);
  }
  // -> hact (EBC_HUMAN_BY_TYPE: everybody's ORCA velocity; the sweep's phase A replaces those of the humans on `linear`)
  if ((a->human_policy == EBC_HUMAN_ORCA || a->human_policy == EBC_HUMAN_BY_TYPE) && (rc = launch_orca(h)) != EBC_OK) return rc;
  rc = a->human_policy == EBC_HUMAN_LINEAR    ? launch_lookahead<EBC_HUMAN_LINEAR>(h, io)
       : a->human_policy == EBC_HUMAN_BY_TYPE ? launch_lookahead<EBC_HUMAN_BY_TYPE>(h, io)
                                              : launch_lookahead<EBC_HUMAN_EXTERNAL>(h, io);
  if (rc != EBC_OK) return rc;
  if (a->location != EBC_DEVICE) return st.finish();
  return EBC_OK;
}

int ebc_row_counts(void *handle, int location, long long *n_rows) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  if (!h->has_reset) return fail(EBC_ERR_STATE, "ebc_row_counts before ebc_reset");
  if (h->faulted) return fail(EBC_ERR_STATE, "ebc_row_counts: the handle reported a mailbox fault; ebc_reset re-arms it");
  if (!n_rows) return fail(EBC_ERR_INVALID, "null n_rows");
  long long *d = n_rows;
  Stager st{h};
  if (location != EBC_DEVICE) {
    if ((rc = ensure_stage(h, pad256((size_t)h->s.E * 8) + 1024)) != EBC_OK) return rc;
    d = st.out(n_rows, (size_t)h->s.E);
  }
  hipLaunchKernelGGL(ebc::row_counts_kernel, dim3((unsigned)((h->s.E + 255) / 256)), dim3(256), 0, h->stream, h->s, d);
  HIP_TRY(hipGetLastError());
  if (location != EBC_DEVICE) return st.finish();
  return EBC_OK;
}

// ebc_observe_wide and ebc_observe_wide_sorted: the same checks, refusals and states, under the entry's own name
static int observe_wide_entry(void *handle, const EbcOmSpec *spec, float *state_wide, long long *n_rows, bool sorted) {
  const std::string who = sorted ? "ebc_observe_wide_sorted" : "ebc_observe_wide";
  if (!spec || spec->struct_size != sizeof(EbcOmSpec)) return fail(EBC_ERR_INVALID, "EbcOmSpec.struct_size");
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  if (!h->has_reset) return fail(EBC_ERR_STATE, who + " before ebc_reset");
  if (h->faulted) return fail(EBC_ERR_STATE, who + ": the handle reported a mailbox fault; ebc_reset re-arms it");
  if (!state_wide) return fail(EBC_ERR_INVALID, who + ": state_wide is NULL");
  if ((rc = check_om_spec(h, spec, who.c_str())) != EBC_OK) return rc;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(h->stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone)
    return fail(EBC_ERR_UNSUPPORTED, who + ": the stream is being captured into a HIP graph; the maps must be launched, not replayed");
  return launch_observe_wide(h, *spec, state_wide, n_rows, sorted);
}

int ebc_observe_wide(void *handle, const EbcOmSpec *spec, float *state_wide, long long *n_rows) {
  return observe_wide_entry(handle, spec, state_wide, n_rows, false);
}

int ebc_observe_wide_sorted(void *handle, const EbcOmSpec *spec, float *state_wide, long long *n_rows) {
  return observe_wide_entry(handle, spec, state_wide, n_rows, true);
}

int ebc_il_targets(void *stream, const double *reward, const uint8_t *done, const uint8_t *info, int K, int E,
                   double gamma_bar, double *values, uint8_t *keep) {
  if (!reward || !done || !info || !values || !keep || K <= 0 || E <= 0) return fail(EBC_ERR_INVALID, "il_targets arguments");
  hipLaunchKernelGGL(ebc::il_targets_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, (hipStream_t)stream, reward, done,
                     info, K, E, gamma_bar, values, keep);
  HIP_TRY(hipGetLastError());
  return EBC_OK;
}

int ebc_get_state(void *handle, const EbcStateView *v) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  if (!v || v->struct_size != sizeof(EbcStateView)) return fail(EBC_ERR_INVALID, "EbcStateView.struct_size");
  const DevState &s = h->s;
  const size_t E = s.E, EN = (size_t)s.E * s.N;
  const hipMemcpyKind kind = v->location == EBC_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
#define CP_(dst, src, bytes) if (dst) HIP_TRY(hipMemcpyAsync((dst), (src), (bytes), kind, h->stream))
  CP_(v->px, s.px, EN * 8); CP_(v->py, s.py, EN * 8); CP_(v->vx, s.vx, EN * 8); CP_(v->vy, s.vy, EN * 8);
  CP_(v->gx, s.gx, EN * 8); CP_(v->gy, s.gy, EN * 8); CP_(v->radius, s.radius, EN * 8);
  CP_(v->v_pref, s.v_pref, EN * 8); CP_(v->type, s.type, EN); CP_(v->n_humans, s.n_humans, E * 4);
  CP_(v->robot, s.robot, E * 9 * 8); CP_(v->global_time, s.time, E * 8);
  CP_(v->arrival_time, s.arrival, EN * 8); CP_(v->done, s.done, E);
#undef CP_
  if (v->location != EBC_DEVICE) HIP_TRY(hipStreamSynchronize(h->stream));
  return EBC_OK;
}

int ebc_timing(void *handle, int enable) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  h->timing = enable != 0;
  return EBC_OK;
}

int ebc_timing_read(void *handle, int reset, double *avg_ms, int64_t *launches) {
  Handle *h;
  int rc = check_handle(handle, &h);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (size_t q = 0; q + 1 < h->ev_used; q += 2) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev[q], h->ev[q + 1]));
    h->ms_sum += ms;
    h->launches += 1;
  }
  h->ev_used = 0;
  if (avg_ms) *avg_ms = h->launches ? h->ms_sum / (double)h->launches : 0.0;
  if (launches) *launches = h->launches;
  if (reset) {
    h->ms_sum = 0;
    h->launches = 0;
  }
  return EBC_OK;
}

}  // extern "C"

#ifdef EBC_WAVE_TRACE
// tools only (libebcsim_trace.so): where the kernels leave their wave timeline, [4][blocks][EBC_TRACE_ROW] u64
extern "C" int ebc_debug_wave_trace(void *device_buffer, unsigned blocks) {
  unsigned long long *b = (unsigned long long *)device_buffer;
  if (hipMemcpyToSymbol(HIP_SYMBOL(ebc::g_wave_trace), &b, sizeof(b)) != hipSuccess) return EBC_ERR_DEVICE;
  if (hipMemcpyToSymbol(HIP_SYMBOL(ebc::g_wave_trace_blocks), &blocks, sizeof(blocks)) != hipSuccess) return EBC_ERR_DEVICE;
  return EBC_OK;
}
// tests only: from the next fused ORCA step on, the ORCA group of flat human index `human` (e * N + i) does
// not publish its velocity, so its consumers run into EBC_SPIN_LIMIT (lowered in this build); -1 = off
extern "C" int ebc_debug_withhold(int human) {
  if (hipMemcpyToSymbol(HIP_SYMBOL(ebc::g_withhold_human), &human, sizeof(human)) != hipSuccess) return EBC_ERR_DEVICE;
  return EBC_OK;
}
#endif
