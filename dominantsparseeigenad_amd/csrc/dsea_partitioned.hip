// dsea_partitioned.hip -- row-partitioned solvers with the collectives inside the library (include/dsea.h,
// "row-partitioned solvers").  Host code + one tiny kernel: the slab kernels are
// the phase kernels of the one-GPU path (dsea_lanczos_kernels.hip, dsea_vector_kernels.hip, dsea_spmv.hip) reached
// through the C ABI of dsea_capi.hip; what this file adds is the SEQUENCING of a distributed Lanczos step / CG iteration -- kernels and RCCL calls issued back to back on the
// caller's stream (slab exchange on a side stream), no host language and no host synchronisation in between.
//
// RCCL is bound at run time (dlopen of the copy already in the process -- PyTorch-ROCm ships and loads its own --
// so that adopted ncclComm_t values are used with the library that created them).
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <new>

#include "dsea_internal.h"

using namespace dsea;

namespace {
struct Rccl {
  bool ok = false;
  decltype(&ncclGetUniqueId) get_unique_id = nullptr;
  decltype(&ncclCommInitRank) comm_init_rank = nullptr;
  decltype(&ncclCommDestroy) comm_destroy = nullptr;
  decltype(&ncclAllReduce) all_reduce = nullptr;
  decltype(&ncclSend) send = nullptr;
  decltype(&ncclRecv) recv = nullptr;
  decltype(&ncclGroupStart) group_start = nullptr;
  decltype(&ncclGroupEnd) group_end = nullptr;
  decltype(&ncclCommCount) comm_count = nullptr;
  decltype(&ncclCommUserRank) comm_user_rank = nullptr;
};
Rccl g_rccl;
std::once_flag g_rccl_once;

void rccl_init() {
  void* lib = nullptr;
  // DSEA_RCCL_LIB=<path>: bind THAT library and nothing else (RTLD_LOCAL: its nccl* symbols do not interpose on the
  // RCCL PyTorch uses).  What the tests use to run the RCCL branch with several ranks on one GPU (tests/fake_rccl).
  const char* forced = getenv("DSEA_RCCL_LIB");
  if (forced && *forced) {
    lib = dlopen(forced, RTLD_NOW | RTLD_LOCAL);
    if (!lib) {
      fprintf(stderr, "libdsea: DSEA_RCCL_LIB=%s cannot be loaded (%s)\n", forced, dlerror());
      return;
    }
  }
  const char* names[] = {"librccl.so", "librccl.so.1"};
  for (const char* nm : names)
    if (!lib) lib = dlopen(nm, RTLD_NOW | RTLD_NOLOAD);      // the copy the process already uses (PyTorch's)
  for (const char* nm : names)
    if (!lib) lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
  if (!lib) return;
#define BIND(field, name)                                                     \
  g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(dlsym(lib, name)); \
  if (!g_rccl.field) return;
  BIND(get_unique_id, "ncclGetUniqueId")
  BIND(comm_init_rank, "ncclCommInitRank")
  BIND(comm_destroy, "ncclCommDestroy")
  BIND(all_reduce, "ncclAllReduce")
  BIND(send, "ncclSend")
  BIND(recv, "ncclRecv")
  BIND(group_start, "ncclGroupStart")
  BIND(group_end, "ncclGroupEnd")
  BIND(comm_count, "ncclCommCount")
  BIND(comm_user_rank, "ncclCommUserRank")
#undef BIND
  g_rccl.ok = true;
}
bool rccl_available() {
  std::call_once(g_rccl_once, rccl_init);
  return g_rccl.ok;
}
}  // namespace

enum CommKind { COMM_RCCL_OWNED = 0, COMM_RCCL_ADOPTED = 1, COMM_CALLBACKS = 2, COMM_SELF = 3 };
struct dsea_comm_s {
  int kind, rank, world;
  ncclComm_t coll, xchg;
  dsea_allreduce_fn allreduce;
  dsea_alltoall_fn alltoall;
  dsea_sendrecv_fn sendrecv;
  void* user;
};

struct dsea_pop_s {
  OpKind kind;
  dsea_comm_s* comm;
  dsea_op_s local;        // slab-local operator
  int64_t nloc;
  int flags;
  double tau;
  // TFIM
  int L, p;
  const double* g_dev;
  double g_const;         // remote part: y += -(g_dev ? *g_dev : 1) * g_scale * sum(partner slabs)
  bool transposed;
  double *xT, *zT, *z, *recv[8], *r_send;
  hipStream_t side;
  hipEvent_t ev_ready, ev_done;
  // stencil
  double* halo;
  bool has_lo, has_hi;
};

namespace {
#define NCCL_OK(call)                      \
  do {                                     \
    if ((call) != ncclSuccess) return DSEA_ERR_COMM; \
  } while (0)

// ---- collectives on one communicator ------------------------------------------------------------------------------
int comm_allreduce(dsea_comm_s* c, double* buf, int64_t count, hipStream_t st) {
  if (c->world == 1 && c->kind != COMM_RCCL_OWNED && c->kind != COMM_RCCL_ADOPTED) return DSEA_OK;
  if (c->kind == COMM_CALLBACKS) return c->allreduce(c->user, buf, count, (void*)st) == 0 ? DSEA_OK : DSEA_ERR_COMM;
  // (world size 1 over RCCL: the call is still issued -- it is what the one-GPU tests exercise)
  NCCL_OK(g_rccl.all_reduce(buf, buf, (size_t)count, ncclDouble, ncclSum, c->coll, st));
  return DSEA_OK;
}

int comm_alltoall(dsea_comm_s* c, const double* send, double* recv, int64_t chunk, hipStream_t st) {
  if (c->kind == COMM_CALLBACKS)
    return c->alltoall(c->user, send, recv, chunk, (void*)st) == 0 ? DSEA_OK : DSEA_ERR_COMM;
  if (c->kind == COMM_SELF || c->world == 1) {
    HIP_TRY(hipMemcpyAsync(recv, send, (size_t)chunk * c->world * sizeof(double), hipMemcpyDeviceToDevice, st));
    return DSEA_OK;
  }
  // an all-to-all IS this group of point-to-point operations; the own chunk is a device copy
  HIP_TRY(hipMemcpyAsync(recv + (int64_t)c->rank * chunk, send + (int64_t)c->rank * chunk, (size_t)chunk * sizeof(double),
                         hipMemcpyDeviceToDevice, st));
  NCCL_OK(g_rccl.group_start());
  bool ok = true;                                            // (a failed call must not leave the group open)
  for (int j = 0; j < c->world && ok; ++j) {
    if (j == c->rank) continue;
    ok = g_rccl.send(send + (int64_t)j * chunk, (size_t)chunk, ncclDouble, j, c->xchg, st) == ncclSuccess &&
         g_rccl.recv(recv + (int64_t)j * chunk, (size_t)chunk, ncclDouble, j, c->xchg, st) == ncclSuccess;
  }
  const bool closed = g_rccl.group_end() == ncclSuccess;
  return ok && closed ? DSEA_OK : DSEA_ERR_COMM;
}

struct P2P {
  const double* send;
  double* recv;
  int64_t count;
  int peer;
};
int comm_sendrecv(dsea_comm_s* c, const P2P* items, int n_items, hipStream_t st) {
  if (n_items == 0) return DSEA_OK;
  if (c->kind == COMM_CALLBACKS) {
    for (int k = 0; k < n_items; ++k)
      if (c->sendrecv(c->user, items[k].send, items[k].recv, items[k].count, items[k].peer, (void*)st) != 0)
        return DSEA_ERR_COMM;
    return DSEA_OK;
  }
  NCCL_OK(g_rccl.group_start());
  bool ok = true;
  for (int k = 0; k < n_items && ok; ++k)
    ok = g_rccl.send(items[k].send, (size_t)items[k].count, ncclDouble, items[k].peer, c->xchg, st) == ncclSuccess &&
         g_rccl.recv(items[k].recv, (size_t)items[k].count, ncclDouble, items[k].peer, c->xchg, st) == ncclSuccess;
  const bool closed = g_rccl.group_end() == ncclSuccess;
  return ok && closed ? DSEA_OK : DSEA_ERR_COMM;
}

int comm_allgather(dsea_comm_s* c, const double* send, double* recv, int64_t count, hipStream_t st) {
  HIP_TRY(hipMemcpyAsync(recv + (int64_t)c->rank * count, send, (size_t)count * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (c->world == 1) return DSEA_OK;
  P2P items[256];
  if (c->world > 256) return DSEA_ERR_ARG;
  int n = 0;
  // round s pairs rank r with (s - r) mod world: a perfect matching per round, every pair exactly once over the rounds --
  // with blocking pairwise callbacks every rank walks the rounds in the same order; over RCCL it is one group
  for (int s = 0; s < c->world; ++s) {
    const int peer = ((s - c->rank) % c->world + c->world) % c->world;
    if (peer != c->rank) items[n++] = P2P{send, recv + (int64_t)peer * count, count, peer};
  }
  return comm_sendrecv(c, items, n, st);
}

// ---- the overlap premise, on the device -----------------------------------------------------------------------------
// rec[0] = first step i at which max_j c_j^2 > tau^2 * c[i] (c[i] = ||r||^2), 0 = never.  c is replicated (it has
// been all-reduced), so every rank records the same step.
__global__ __launch_bounds__(256) void k_premise(const double* __restrict__ c, int i, double tau, double* __restrict__ rec) {
  __shared__ double sm[256];
  double m = 0.0;
  for (int j = threadIdx.x; j < i; j += 256) {
    const double v = c[j] * c[j];
    m = v > m ? v : m;
  }
  sm[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) sm[threadIdx.x] = sm[threadIdx.x] > sm[threadIdx.x + s] ? sm[threadIdx.x] : sm[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double rr = c[i];
    const bool ok = sm[0] <= tau * tau * rr;      // NaN -> violated
    if (!ok && rec[0] == 0.0) rec[0] = (double)i;
  }
}

// ---- TFIM slab exchange ------------------------------------------------------------------------------------------
int tfim_exchange_on(dsea_pop_s* P, const double* x, hipStream_t s) {
  dsea_comm_s* c = P->comm;
  if (P->transposed) {
    const int64_t chunk = P->nloc / c->world;
    DSEA_TRY(comm_alltoall(c, x, P->xT, chunk, s));
    DSEA_TRY(dsea_hypercube_flipsum(P->xT, P->zT, c->world, chunk, (void*)s));
    DSEA_TRY(comm_alltoall(c, P->zT, P->z, chunk, s));
    return DSEA_OK;
  }
  P2P items[8];
  for (int b = 0; b < P->p; ++b) items[b] = P2P{x, P->recv[b], P->nloc, c->rank ^ (1 << b)};
  return comm_sendrecv(c, items, P->p, s);
}
// start the exchange of slab x: on the side stream (ordered after what `main` has enqueued so far) when there is one,
// otherwise inline on main.  x must stay untouched until tfim_exchange_finish.
int tfim_exchange_start(dsea_pop_s* P, const double* x, hipStream_t main) {
  if (P->p == 0 || (P->flags & DSEA_POP_NO_EXCHANGE)) return DSEA_OK;
  if (!P->side) return tfim_exchange_on(P, x, main);
  HIP_TRY(hipEventRecord(P->ev_ready, main));
  HIP_TRY(hipStreamWaitEvent(P->side, P->ev_ready, 0));
  DSEA_TRY(tfim_exchange_on(P, x, P->side));
  HIP_TRY(hipEventRecord(P->ev_done, P->side));
  return DSEA_OK;
}
int tfim_exchange_finish(dsea_pop_s* P, hipStream_t main) {
  if (P->p == 0 || !P->side || (P->flags & DSEA_POP_NO_EXCHANGE)) return DSEA_OK;
  HIP_TRY(hipStreamWaitEvent(main, P->ev_done, 0));
  return DSEA_OK;
}
inline int tfim_recv_list(dsea_pop_s* P, const double** out) {
  if (P->p == 0) return 0;
  if (P->transposed) {
    out[0] = P->z;
    return 1;
  }
  for (int b = 0; b < P->p; ++b) out[b] = P->recv[b];
  return P->p;
}
// remote part of the mat-vec + shift + LOCAL x.y into dot_local
int tfim_remote_part(dsea_pop_s* P, dsea_ws_t ws, const double* shift, const double* skip, const double* x, double* y,
                     double* dot_local, hipStream_t st) {
  const double* xs[8];
  const int cnt = tfim_recv_list(P, xs);
  return dsea_axpy_multi_dot(ws, P->g_dev ? -1.0 : -P->g_const, P->g_dev, xs, cnt, shift, skip, x, y, P->nloc, dot_local,
                             (void*)st);
}

int stencil_halo_exchange(dsea_pop_s* P, const double* x, hipStream_t st) {
  P2P items[2];
  int n = 0;
  if (P->has_lo) items[n++] = P2P{x, P->halo, 1, P->comm->rank - 1};
  if (P->has_hi) items[n++] = P2P{x + (P->nloc - 1), P->halo + 1, 1, P->comm->rank + 1};
  return comm_sendrecv(P->comm, items, n, st);
}

// explicit-matrix slab (dsea_pop_create_csr): hb elements with each neighbour, or the all-gather fallback
int sell_halo_exchange(dsea_pop_s* P, const double* x, hipStream_t st) {
  const SellParams& p = P->local.d.sell;
  if (p.mode == 2) return comm_allgather(P->comm, x, const_cast<double*>(p.xg), P->nloc, st);
  if (p.hb == 0) return DSEA_OK;
  P2P items[2];
  int n = 0;
  if (P->has_lo) items[n++] = P2P{x, const_cast<double*>(p.halo_lo), p.hb, P->comm->rank - 1};
  if (P->has_hi) items[n++] = P2P{x + (P->nloc - p.hb), const_cast<double*>(p.halo_hi), p.hb, P->comm->rank + 1};
  return comm_sendrecv(P->comm, items, n, st);
}
inline int halo_exchange(dsea_pop_s* P, const double* x, hipStream_t st) {
  return P->kind == OP_SELL ? sell_halo_exchange(P, x, st) : stencil_halo_exchange(P, x, st);
}

// y = (A - shift) x over all ranks, LOCAL x.y into dot_local (ws scalar)
int pop_apply(dsea_pop_s* P, dsea_ws_t ws, const double* x, double* y, const double* shift, const double* skip,
              double* dot_local, hipStream_t st) {
  if (P->kind == OP_TFIM && P->p == 0)   // one rank: nothing to exchange, shift and dot ride on the mat-vec itself
    return dsea_spmv(&P->local, ws, x, y, shift, dot_local, skip, (void*)st);
  if (P->kind == OP_TFIM) {
    DSEA_TRY(tfim_exchange_start(P, x, st));
    DSEA_TRY(dsea_spmv(&P->local, nullptr, x, y, nullptr, nullptr, skip, (void*)st));
    DSEA_TRY(tfim_exchange_finish(P, st));
    return tfim_remote_part(P, ws, shift, skip, x, y, dot_local, st);
  }
  DSEA_TRY(halo_exchange(P, x, st));
  return dsea_spmv(&P->local, ws, x, y, shift, dot_local, skip, (void*)st);
}
// ---- CG on the reference's recurrences (CG.py:24-41 distributed): one exchange and two scalar all-reduces per iteration ----
int pop_cg_run_reference(dsea_pop_s* P, dsea_ws_t ws, const double* shift, const double* b, double* x, double* state,
                         double eps, int64_t maxiter, int poll_every, int64_t* iters_out, double* resnorm_out, hipStream_t st) {
  const int64_t n = P->nloc;
  Workspace& w = ws->w;
  void* stream = (void*)st;
  double* r = w.vec[1];
  double* d = w.vec[2];
  double* Ad = w.vec[3];
  const double* done = state + DSEA_CG_DONE;
  // r = b - A'x0 ; early out ; d = r                                   (CG.py:26-30)
  DSEA_TRY(pop_apply(P, ws, x, Ad, shift, nullptr, w.scal + 36, st));
  DSEA_TRY(dsea_cg_init(ws, b, Ad, r, d, state, n, stream));
  DSEA_TRY(comm_allreduce(P->comm, state + DSEA_CG_RR, 1, st));
  DSEA_TRY(dsea_cg_init_check(ws, state, eps, stream));
  double host_state[DSEA_CG_STATE_LEN];
  DSEA_TRY(read_to_host(host_state, state, sizeof(host_state), st));
  auto iterations = [&](int64_t, int64_t count) -> int {
    for (int64_t it = 0; it < count; ++it) {
      DSEA_TRY(pop_apply(P, ws, d, Ad, shift, done, state + DSEA_CG_DAD, st));          // A'd, local d.A'd  (CG.py:31/40)
      DSEA_TRY(comm_allreduce(P->comm, state + DSEA_CG_DAD, 1, st));
      DSEA_TRY(dsea_cg_update(ws, x, r, d, Ad, state, n, stream));                       // CG.py:31,33-34
      DSEA_TRY(comm_allreduce(P->comm, state + DSEA_CG_RRNEW, 1, st));
      DSEA_TRY(dsea_cg_check(ws, state, eps, stream));                                   // CG.py:35-38
      DSEA_TRY(dsea_cg_direction(ws, r, d, state, n, stream));                           // CG.py:39
    }
    return DSEA_OK;
  };
  // blocking polls: a chunk issued after convergence would still run its collectives
  if (host_state[DSEA_CG_DONE] == 0.0 && maxiter > 0)
    DSEA_TRY(cg_poll(state, host_state, maxiter, poll_every, nullptr, iterations, st));
  return cg_result(host_state, iters_out, resnorm_out);
}

// ---- CG with ONE all-reduce per iteration (Chronopoulos-Gear; kernels: k_pcg_update / k_pcg_scalars) ------------------
// per iteration: [p, s, x, r update + local r.r partials] -> mat-vec w = A'r with its exchange (+ local r.w; the SAME
// launch closes both local sums) -> all-reduce(gamma', delta) -> scalars (stopping test, beta, alpha).  Four launches
// and one all-reduce where the reference's recurrences need seven and two.
//
// TRUE-RESIDUAL CHECK (round-5 advisor, medium).  Both r and s = A'p are carried by recurrences here, and Chronopoulos-Gear
// is known to lose attainable accuracy against standard CG: the recursive ||r|| can pass the stopping test while b - A'x is
// still above it.  A stop is therefore only accepted after r = b - A'x has been recomputed from x (one extra mat-vec and
// all-reduce per solve) and found below eps -- which is simply the first thing a RESTART from x does.  If it is not, the
// restart continues (residual replacement: the recurrences start again from the true residual); after
// DSEA_PCG_MAX_RESTARTS of those the solve is finished on the reference's recurrences from the current x.  resnorm_out is
// the TRUE residual whenever the solve converged on this path.
#define DSEA_PCG_MAX_RESTARTS 3
int pop_cg_run_one_reduction(dsea_pop_s* P, dsea_ws_t ws, const double* shift, const double* b, double* x, double* state,
                             double eps, int64_t maxiter, int poll_every, int64_t* iters_out, double* resnorm_out,
                             hipStream_t st) {
  const int64_t n = P->nloc;
  Workspace& w = ws->w;
  double* s = w.vec[0];
  double* r = w.vec[1];
  double* p = w.vec[2];
  double* wv = w.vec[3];
  double* pair = w.scal + 32;                                   // (gamma', delta): local sums, then all-reduced in place
  double* rrP = w.aux + 3 * DSEA_MAX_WAVE_TILES;                // partials of r.r left by k_pcg_update
  const double* done = state + DSEA_CG_DONE;
  // the pending-partials hand-off to the mat-vec's dot-closing launch must not survive an early error return: the next
  // dsea_spmv / dsea_axpy_multi_dot on this workspace would fold stale partials into a stale slot (round-5 advisor, low)
  struct PendGuard {
    Workspace& w;
    explicit PendGuard(Workspace& ww) : w(ww) { w.pend_P = nullptr; }
    ~PendGuard() { w.pend_P = nullptr; }
  } pend_guard(w);
  auto iterations = [&](int64_t, int64_t count) -> int {
    for (int64_t it = 0; it < count; ++it) {
      const int nb = launch_pcg_update(x, r, p, s, wv, state, n, rrP, st);
      w.pend_P = rrP;                                             // closed by the mat-vec's own dot-closing launch
      w.pend_count = nb;
      w.pend_out = pair;
      DSEA_TRY(pop_apply(P, ws, r, wv, shift, done, pair + 1, st));
      if (w.pend_P) {
        launch_finalize1(w.pend_P, w.pend_count, w.pend_out, st);
        w.pend_P = nullptr;
      }
      DSEA_TRY(comm_allreduce(P->comm, pair, 2, st));
      launch_pcg_scalars(state, pair, eps, 0, st);
    }
    return DSEA_OK;
  };
  double host_state[DSEA_CG_STATE_LEN];
  int64_t total_iters = 0;
  for (int attempt = 0;; ++attempt) {
    // r = b - A'x (the TRUE residual of the current x) ; early out / acceptance of the previous attempt's stop   (CG.py:26-29)
    DSEA_TRY(pop_apply(P, ws, x, wv, shift, nullptr, w.scal + 36, st));
    DSEA_TRY(dsea_cg_init(ws, b, wv, r, p, state, n, (void*)st));       // (p = r: what beta = 0 makes of it anyway)
    DSEA_TRY(comm_allreduce(P->comm, state + DSEA_CG_RR, 1, st));
    DSEA_TRY(dsea_cg_init_check(ws, state, eps, (void*)st));
    DSEA_TRY(read_to_host(host_state, state, sizeof(host_state), st));
    if (host_state[DSEA_CG_DONE] != 0.0 || total_iters >= maxiter) break;
    if (attempt > DSEA_PCG_MAX_RESTARTS) {
      // the one-reduction recurrences keep stopping above the true tolerance: finish on the reference's
      int64_t it2 = 0;
      const int rc = pop_cg_run_reference(P, ws, shift, b, x, state, eps, maxiter - total_iters, poll_every, &it2, resnorm_out, st);
      if (iters_out) *iters_out = total_iters + it2;
      return rc;
    }
    HIP_TRY(hipMemsetAsync(s, 0, (size_t)n * sizeof(double), st));
    // w = A'r, delta = r.w ; alpha = gamma / delta, beta = 0
    DSEA_TRY(pop_apply(P, ws, r, wv, shift, done, pair + 1, st));
    DSEA_TRY(comm_allreduce(P->comm, pair + 1, 1, st));
    launch_pcg_scalars(state, pair, eps, 1, st);
    DSEA_TRY(cg_poll(state, host_state, maxiter - total_iters, poll_every, nullptr, iterations, st));   // (blocking, as above)
    total_iters += (int64_t)host_state[DSEA_CG_ITERS];
    if (host_state[DSEA_CG_DONE] == 0.0) break;                     // iteration budget spent
    // the recursive residual passed the test: the next round's first step recomputes the true one and decides
  }
  const int rc = cg_result(host_state, nullptr, resnorm_out);
  if (iters_out) *iters_out = total_iters;
  return rc;
}
}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------------------- communicator
int dsea_comm_unique_id(void* id_out) {
  if (!id_out) return DSEA_ERR_ARG;
  if (!rccl_available()) return DSEA_ERR_UNSUPPORTED;
  static_assert(sizeof(ncclUniqueId) == DSEA_COMM_ID_BYTES, "unique id size");
  ncclUniqueId id;
  NCCL_OK(g_rccl.get_unique_id(&id));
  memcpy(id_out, &id, sizeof(id));
  return DSEA_OK;
}

int dsea_comm_init_rank(const void* id_coll, const void* id_xchg, int rank, int world, dsea_comm_t* out) {
  if (!id_coll || !out || world < 1 || rank < 0 || rank >= world) return DSEA_ERR_ARG;
  if (!rccl_available()) return DSEA_ERR_UNSUPPORTED;
  dsea_comm_s* c = new (std::nothrow) dsea_comm_s;
  if (!c) return DSEA_ERR_ARG;
  memset(c, 0, sizeof(*c));
  c->kind = COMM_RCCL_OWNED;
  c->rank = rank;
  c->world = world;
  ncclUniqueId id;
  memcpy(&id, id_coll, sizeof(id));
  if (g_rccl.comm_init_rank(&c->coll, world, id, rank) != ncclSuccess) {
    delete c;
    return DSEA_ERR_COMM;
  }
  c->xchg = c->coll;
  if (id_xchg) {
    memcpy(&id, id_xchg, sizeof(id));
    if (g_rccl.comm_init_rank(&c->xchg, world, id, rank) != ncclSuccess) {
      g_rccl.comm_destroy(c->coll);
      delete c;
      return DSEA_ERR_COMM;
    }
  }
  *out = c;
  return DSEA_OK;
}

int dsea_comm_adopt(void* coll_comm, void* xchg_comm, int rank, int world, dsea_comm_t* out) {
  if (!coll_comm || !out || world < 1 || rank < 0 || rank >= world) return DSEA_ERR_ARG;
  if (!rccl_available()) return DSEA_ERR_UNSUPPORTED;
  ncclComm_t cc = static_cast<ncclComm_t>(coll_comm);
  int cnt = -1, ur = -1;
  // the adopted handle must be a live communicator of this size and rank (a stale or foreign pointer fails here)
  if (g_rccl.comm_count(cc, &cnt) != ncclSuccess || g_rccl.comm_user_rank(cc, &ur) != ncclSuccess) return DSEA_ERR_COMM;
  if (cnt != world || ur != rank) return DSEA_ERR_ARG;
  dsea_comm_s* c = new (std::nothrow) dsea_comm_s;
  if (!c) return DSEA_ERR_ARG;
  memset(c, 0, sizeof(*c));
  c->kind = COMM_RCCL_ADOPTED;
  c->rank = rank;
  c->world = world;
  c->coll = cc;
  c->xchg = xchg_comm ? static_cast<ncclComm_t>(xchg_comm) : cc;
  *out = c;
  return DSEA_OK;
}

int dsea_comm_create_callbacks(int rank, int world, dsea_allreduce_fn allreduce, dsea_alltoall_fn alltoall,
                               dsea_sendrecv_fn sendrecv, void* user, dsea_comm_t* out) {
  if (!out || world < 1 || rank < 0 || rank >= world) return DSEA_ERR_ARG;
  if (world > 1 && (!allreduce || !alltoall || !sendrecv)) return DSEA_ERR_ARG;
  dsea_comm_s* c = new (std::nothrow) dsea_comm_s;
  if (!c) return DSEA_ERR_ARG;
  memset(c, 0, sizeof(*c));
  c->kind = (world == 1 && !allreduce) ? COMM_SELF : COMM_CALLBACKS;
  c->rank = rank;
  c->world = world;
  c->allreduce = allreduce;
  c->alltoall = alltoall;
  c->sendrecv = sendrecv;
  c->user = user;
  *out = c;
  return DSEA_OK;
}

int dsea_comm_destroy(dsea_comm_t c) {
  if (!c) return DSEA_OK;
  if (c->kind == COMM_RCCL_OWNED && g_rccl.ok) {
    if (c->xchg && c->xchg != c->coll) g_rccl.comm_destroy(c->xchg);
    if (c->coll) g_rccl.comm_destroy(c->coll);
  }
  delete c;
  return DSEA_OK;
}

int dsea_comm_allreduce(dsea_comm_t comm, double* buf, int64_t count, void* stream) {
  if (!comm || !buf || count < 1) return DSEA_ERR_ARG;
  return comm_allreduce(comm, buf, count, static_cast<hipStream_t>(stream));
}

int dsea_comm_alltoall(dsea_comm_t comm, const double* send, double* recv, int64_t chunk, void* stream) {
  if (!comm || !send || !recv || chunk < 1 || send == recv) return DSEA_ERR_ARG;
  return comm_alltoall(comm, send, recv, chunk, static_cast<hipStream_t>(stream));
}

int dsea_comm_allgather(dsea_comm_t comm, const double* send, double* recv, int64_t count, void* stream) {
  if (!comm || !send || !recv || count < 1) return DSEA_ERR_ARG;
  return comm_allgather(comm, send, recv, count, static_cast<hipStream_t>(stream));
}

// ---------------------------------------------------------------------------------------------- operators
size_t dsea_pop_tfim_scratch_doubles(int L, int world) {
  if (L < 1 || L > 62 || world < 1) return 0;
  int p = 0;
  while ((1 << p) < world) ++p;
  if ((1 << p) != world || p > L) return 0;
  const size_t nloc = (size_t)1 << (L - p);
  return (size_t)((p > 3 ? p : 3) + 1) * nloc;
}

int dsea_pop_create_tfim(int L, dsea_comm_t comm, const double* g_dev, double g_const, double diag_scale,
                         double* scratch, void* side_stream, int flags, double tau, dsea_pop_t* out) {
  if (!out || !comm || L < 1 || L > 62 || tau < 0.0) return DSEA_ERR_ARG;
  int p = 0;
  while ((1 << p) < comm->world) ++p;
  if ((1 << p) != comm->world || p > L || p > 8) return DSEA_ERR_ARG;
  if (p > 0 && !scratch) return DSEA_ERR_ARG;
  if (scratch && !aligned16(scratch)) return DSEA_ERR_ALIGN;
  dsea_pop_s* P = new (std::nothrow) dsea_pop_s;
  if (!P) return DSEA_ERR_ARG;
  memset(static_cast<void*>(P), 0, sizeof(*P));
  P->kind = OP_TFIM;
  P->comm = comm;
  P->L = L;
  P->p = p;
  P->nloc = (int64_t)1 << (L - p);
  P->flags = flags;
  P->tau = tau;
  P->g_dev = g_dev;
  P->g_const = g_const;
  memset(&P->local.d, 0, sizeof(P->local.d));
  P->local.d.tune_tile_log2 = DSEA_TFIM_TILE_LOG2;
  P->local.d.kind = OP_TFIM;
  P->local.d.n = P->nloc;
  P->local.d.tfim = TfimParams{L, L - p, (int64_t)comm->rank * P->nloc, g_dev, g_const, diag_scale};
  // exchange form: pairwise for two ranks (the transposed form would move the same bytes), transposed from four on
  P->transposed = comm->world >= 4 && P->nloc >= comm->world && !(flags & DSEA_POP_PAIRWISE);
  if (p > 0) {
    // scratch layout: [r_send][xT zT z | recv_0 .. recv_{p-1}]   (both forms fit: (max(3, p) + 1) slabs)
    P->r_send = scratch;
    double* base = scratch + P->nloc;
    P->xT = base;
    P->zT = base + P->nloc;
    P->z = base + 2 * P->nloc;
    for (int b = 0; b < p; ++b) P->recv[b] = base + (int64_t)b * P->nloc;
  }
  P->side = static_cast<hipStream_t>(side_stream);
  if (P->side) {
    hipError_t e = hipEventCreateWithFlags(&P->ev_ready, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&P->ev_done, hipEventDisableTiming);
    if (e != hipSuccess) {
      delete P;
      return hip_fail(e);
    }
  }
  *out = P;
  return DSEA_OK;
}

int dsea_pop_create_stencil3(int64_t n_local, double coef, const double* V_dev, double* halo2, dsea_comm_t comm,
                             dsea_pop_t* out) {
  if (!out || !comm || n_local < 1 || !V_dev || !halo2) return DSEA_ERR_ARG;
  if (!aligned16(V_dev)) return DSEA_ERR_ALIGN;
  dsea_pop_s* P = new (std::nothrow) dsea_pop_s;
  if (!P) return DSEA_ERR_ARG;
  memset(static_cast<void*>(P), 0, sizeof(*P));
  P->kind = OP_STENCIL3;
  P->comm = comm;
  P->nloc = n_local;
  P->halo = halo2;
  P->has_lo = comm->rank > 0;
  P->has_hi = comm->rank < comm->world - 1;
  memset(&P->local.d, 0, sizeof(P->local.d));
  P->local.d.tune_tile_log2 = DSEA_TFIM_TILE_LOG2;
  P->local.d.kind = OP_STENCIL3;
  P->local.d.n = n_local;
  P->local.d.st3 = Stencil3Params{n_local, coef, V_dev, P->has_lo ? halo2 : nullptr, P->has_hi ? halo2 + 1 : nullptr};
  *out = P;
  return DSEA_OK;
}

int dsea_pop_create_csr(dsea_op_t local_op, dsea_comm_t comm, dsea_pop_t* out) {
  if (!out || !comm || !local_op) return DSEA_ERR_ARG;
  if (local_op->d.kind != OP_SELL) return DSEA_ERR_UNSUPPORTED;
  const SellParams& sp = local_op->d.sell;
  if (sp.mode != 1 && sp.mode != 2) return DSEA_ERR_ARG;       // dsea_op_set_slab first
  dsea_pop_s* P = new (std::nothrow) dsea_pop_s;
  if (!P) return DSEA_ERR_ARG;
  memset(static_cast<void*>(P), 0, sizeof(*P));
  P->kind = OP_SELL;
  P->comm = comm;
  P->nloc = local_op->d.n;
  P->has_lo = comm->rank > 0;
  P->has_hi = comm->rank < comm->world - 1;
  if (sp.mode == 1 && sp.hb > 0 && ((P->has_lo && !sp.halo_lo) || (P->has_hi && !sp.halo_hi))) {
    delete P;
    return DSEA_ERR_ARG;
  }
  P->local = *local_op;                                          // (arrays and exchange buffers stay the caller's)
  *out = P;
  return DSEA_OK;
}

int dsea_pop_sddmm(dsea_pop_t P, const int64_t* rowptr, const double* v1, const double* v2, double alpha, int flags,
                   double* out, void* stream) {
  if (!P || !rowptr || !v1 || !v2 || !out || (flags & ~(DSEA_SDDMM_ACCUMULATE | DSEA_SDDMM_SYMMETRIC))) return DSEA_ERR_ARG;
  if (P->kind != OP_SELL) return DSEA_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int acc = (flags & DSEA_SDDMM_ACCUMULATE) ? 1 : 0;
  const bool sym = (flags & DSEA_SDDMM_SYMMETRIC) != 0;
  // the column operand travels like the x of a mat-vec; the symmetric form is two one-sided launches (one exchange each)
  DSEA_TRY(sell_halo_exchange(P, v2, st));
  if (launch_sddmm(P->local.d, rowptr, v1, v2, sym ? 0.5 * alpha : alpha, acc, false, out, st) != 0) return DSEA_ERR_UNSUPPORTED;
  if (sym) {
    DSEA_TRY(sell_halo_exchange(P, v1, st));
    if (launch_sddmm(P->local.d, rowptr, v2, v1, 0.5 * alpha, 1, false, out, st) != 0) return DSEA_ERR_UNSUPPORTED;
  }
  return check_launch();
}

int dsea_pop_destroy(dsea_pop_t P) {
  if (!P) return DSEA_OK;
  if (P->side) {
    (void)hipEventDestroy(P->ev_ready);
    (void)hipEventDestroy(P->ev_done);
  }
  delete P;
  return DSEA_OK;
}

int dsea_pop_set_flags(dsea_pop_t P, int flags) {
  if (!P) return DSEA_ERR_ARG;
  const bool pairwise = (flags & DSEA_POP_PAIRWISE) != 0;
  if (P->kind == OP_TFIM) P->transposed = P->comm->world >= 4 && P->nloc >= P->comm->world && !pairwise;
  P->flags = flags;
  return DSEA_OK;
}

int dsea_pop_matvec(dsea_pop_t P, dsea_ws_t ws, const double* x, double* y, const double* shift, double* dot_out,
                    const double* skip_flag, void* stream) {
  if (!P || !ws || !x || !y || x == y) return DSEA_ERR_ARG;
  if (!aligned16(x) || !aligned16(y)) return DSEA_ERR_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* slot = dot_out ? dot_out : ws->w.scal + 36;
  DSEA_TRY(pop_apply(P, ws, x, y, shift, skip_flag, slot, st));
  if (dot_out) DSEA_TRY(comm_allreduce(P->comm, dot_out, 1, st));
  return DSEA_OK;
}

int dsea_pop_dot(dsea_pop_t P, dsea_ws_t ws, const double* x, const double* y, int64_t n, double* out, void* stream) {
  if (!P || !ws || !out) return DSEA_ERR_ARG;
  DSEA_TRY(dsea_dot(ws, x, y, n, out, stream));
  return comm_allreduce(P->comm, out, 1, static_cast<hipStream_t>(stream));
}

// ---------------------------------------------------------------------------------------------- Lanczos
int dsea_pop_lanczos_run(dsea_pop_t P, dsea_ws_t ws, int k, const double* q0, double* Q, int64_t ldq, double* alphas,
                         double* betas, void* stream) {
  if (!P || !ws || !q0 || !Q || !alphas || !betas || k < 1) return DSEA_ERR_ARG;
  const int64_t n = P->nloc;
  if (ldq < n || ws->w.n < n) return DSEA_ERR_ARG;
  if (k > ws->w.kmax && k != 1) return DSEA_ERR_WORKSPACE;
  if (!aligned16(q0) || !aligned16(Q) || (ldq % 2) != 0) return DSEA_ERR_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  Workspace& w = ws->w;
  double* u = w.vec[0];
  double* r = w.vec[1];
  double* y = w.vec[2];
  double* c = w.coef;
  double* pair = w.scal + 32;
  double* rec = w.scal + 34;      // overlap premise record
  const bool tfim = P->kind == OP_TFIM;
  // partial re-orthogonalisation (dsea_ws_set_partial_reorth): as in dsea_lanczos_run, with the norm the estimates need
  // closed by one more scalar all-reduce per step; the exchange of the un-corrected r is not overlapped in this mode
  const bool partial = w.partial_reorth != 0;
  const bool overlap = tfim && P->p > 0 && (P->flags & DSEA_POP_OVERLAP) && !partial;
  double* pro_flag = w.scal + DSEA_SCAL_PRO;
  double* pro_rr = w.scal + DSEA_SCAL_PRO + 4;                   // global ||r||^2 of the un-corrected r
  double* pro_om = w.aux + 4 * DSEA_MAX_WAVE_TILES;
  const double pro_eps1 = 64.0 * 2.220446049250313e-16;
  const TileGeom g = w.geom(n);
  // "lite" finish (non-overlapped step, wave-owned geometry): k_plz_finish stores q = r / beta only; u = y / beta is formed by
  // the NEXT step's dots pass while it reads y (k_rdots<., ., USCALE>: the same division, bit-identical) -- one vector
  // written and one read fewer per step than storing u and reading it back
  const char* lite_env = getenv("DSEA_POP_LITE");               // (A/B switch: 0 = store u and read it back)
  const bool lite = !partial && rdots_uscale_ok(g) && !(lite_env && lite_env[0] == '0');
  double* beta0 = w.scal + 37;                                   // beta of step 0 (= ||q0||; betas[] starts at step 1)
  // the step's two local sums (||r||^2 from the correction pass, r.Ar from the mat-vec) are closed by ONE launch
  struct DeferNorm {
    Workspace& w;
    explicit DeferNorm(Workspace& ww) : w(ww) { w.defer_norm = 1; w.pend_P = nullptr; }
    ~DeferNorm() { w.defer_norm = 0; w.pend_P = nullptr; }
  } defer_guard(w);
  HIP_TRY(hipMemsetAsync(w.scal + DSEA_SCAL_PRO, 0, 5 * sizeof(double), st));
  HIP_TRY(hipMemsetAsync(w.scal + 32, 0, 4 * sizeof(double), st));
  HIP_TRY(hipMemsetAsync(w.scal + 16, 0, 2 * sizeof(double), st));      // shadow-path statistics of this run
  for (int i = 0; i < k; ++i) {
    const double* a_prev = i >= 1 ? alphas + (i - 1) : nullptr;
    const double* b_prev = i >= 2 ? betas + (i - 2) : nullptr;
    if (i == 0) {
      HIP_TRY(hipMemcpyAsync(r, q0, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
      if (overlap) {
        HIP_TRY(hipMemcpyAsync(P->r_send, q0, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
        DSEA_TRY(tfim_exchange_start(P, P->r_send, st));
      }
    } else if (overlap) {
      // the exchange of the UN-corrected r runs behind the dots and correction passes; r and its snapshot were formed by
      // the fused tail of the previous step (k_plz_finish_form = k_plz_finish + k_form_r, bit-identical)
      DSEA_TRY(tfim_exchange_start(P, P->r_send, st));
      // alpha = 0: r is rewritten with its own values (read from the snapshot, so that input and output of the
      // kernel do not alias), c = Q^T r, c[i] = r.r
      DSEA_TRY(dsea_plz_dots(ws, Q, ldq, n, i, P->r_send, w.zero, nullptr, r, c, stream));
      DSEA_TRY(comm_allreduce(P->comm, c, i + 1, st));
      hipLaunchKernelGGL(k_premise, dim3(1), dim3(256), 0, st, (const double*)c, i, P->tau, rec);
    } else if (partial && i >= 1) {
      // (1) r = u - alpha q - beta q', local ||r||^2 -> c[i]; (2) its global sum feeds the estimates, which decide on the
      // device (identically on every rank: same scalars); (3) c = Q^T r (copy of r to y, unused) or nothing
      launch_rdots(g, Q, ldq, n, i, u, a_prev, b_prev, r, w.partials, nullptr, st, nullptr, nullptr, 0, nullptr, true,
                   nullptr, w.zero, false);
      launch_finalize1(w.partials + (int64_t)i * g.pstride, rdots_partial_count(g, i), c + i, st);
      HIP_TRY(hipMemcpyAsync(pro_rr, c + i, sizeof(double), hipMemcpyDeviceToDevice, st));
      DSEA_TRY(comm_allreduce(P->comm, pro_rr, 1, st));
      launch_pro_update(alphas, betas, pro_rr, 1, pro_rr, pro_om, DSEA_MAX_WAVE_TILES, pro_flag, pro_flag + 1, i, pro_eps1,
                        w.pro_delta, nullptr, st);
      HIP_TRY(hipMemsetAsync(c, 0, (size_t)i * sizeof(double), st));       // (what the all-reduce sums on the other steps)
      launch_rdots(g, Q, ldq, n, i, r, w.zero, nullptr, y, w.partials, c, st, w.prof ? w.prof->next(PROF_RDOTS) : nullptr,
                   nullptr, 0, nullptr, false, nullptr, pro_flag, true);
      DSEA_TRY(comm_allreduce(P->comm, c, i, st));
      launch_axpy_norm(g, Q, ldq, n, i, c, r, w.partials, pair, st, w.prof ? w.prof->next(PROF_AXPY) : nullptr, nullptr,
                       pro_flag);
    } else if (lite) {
      launch_rdots(g, Q, ldq, n, i, y, a_prev, b_prev, r, w.partials, c, st, w.prof ? w.prof->next(PROF_RDOTS) : nullptr, nullptr,
                   0, nullptr, true, nullptr, nullptr, false, i >= 2 ? betas + (i - 2) : beta0);
      DSEA_TRY(comm_allreduce(P->comm, c, i + 1, st));
    } else {
      DSEA_TRY(dsea_plz_dots(ws, Q, ldq, n, i, u, a_prev, b_prev, r, c, stream));
      DSEA_TRY(comm_allreduce(P->comm, c, i + 1, st));
    }
    if (!(partial && i >= 1)) DSEA_TRY(dsea_plz_correct(ws, Q, ldq, n, i, c, r, pair, stream));
    if (tfim && P->p == 0) {
      DSEA_TRY(dsea_spmv(&P->local, ws, r, y, nullptr, pair + 1, nullptr, stream));
    } else if (tfim) {
      if (!overlap) DSEA_TRY(tfim_exchange_start(P, r, st));       // r is final: exact, runs behind the local mat-vec
      DSEA_TRY(dsea_spmv(&P->local, nullptr, r, y, nullptr, nullptr, nullptr, stream));
      DSEA_TRY(tfim_exchange_finish(P, st));
      DSEA_TRY(tfim_remote_part(P, ws, nullptr, nullptr, r, y, pair + 1, st));
    } else {
      DSEA_TRY(halo_exchange(P, r, st));
      DSEA_TRY(dsea_spmv(&P->local, ws, r, y, nullptr, pair + 1, nullptr, stream));
    }
    if (w.pend_P) {     // (no dot-closing call consumed the deferred ||r||^2 on this path: close it now)
      launch_finalize1(w.pend_P, w.pend_count, w.pend_out, st);
      w.pend_P = nullptr;
    }
    DSEA_TRY(comm_allreduce(P->comm, pair, 2, st));
    if (overlap && i + 1 < k) {
      uint16_t* qs = (w.shadow && w.shadow_rows > i && w.shadow_ld >= n) ? w.shadow + (int64_t)i * w.shadow_ld : nullptr;
      launch_plz_finish_form(r, y, pair, Q + (int64_t)i * ldq, qs, i >= 1 ? Q + (int64_t)(i - 1) * ldq : nullptr, alphas + i,
                             i >= 1 ? betas + (i - 1) : nullptr, P->r_send, n, st);
    } else if (lite && !overlap) {
      uint16_t* qs = (w.shadow && w.shadow_rows > i && w.shadow_ld >= n) ? w.shadow + (int64_t)i * w.shadow_ld : nullptr;
      launch_plz_finish(r, y, pair, Q + (int64_t)i * ldq, qs, nullptr, alphas + i, i >= 1 ? betas + (i - 1) : beta0, n, st);
    } else {
      DSEA_TRY(dsea_plz_finish(ws, r, y, pair, Q + (int64_t)i * ldq, i, u, alphas + i, i >= 1 ? betas + (i - 1) : nullptr, n,
                               stream));
    }
  }
  return check_launch();
}

int dsea_pop_lanczos_status(dsea_pop_t P, dsea_ws_t ws, int* step, void* stream) {
  if (!P || !ws) return DSEA_ERR_ARG;
  double h = 0.0;
  DSEA_TRY(read_to_host(&h, ws->w.scal + 34, sizeof(h), static_cast<hipStream_t>(stream)));
  if (step) *step = (int)h;
  return h != 0.0 ? DSEA_ERR_PREMISE : DSEA_OK;
}

// ---------------------------------------------------------------------------------------------- CG
int dsea_pop_cg_run(dsea_pop_t P, dsea_ws_t ws, const double* shift, const double* b, double* x, double* state,
                    double eps, int64_t maxiter, int poll_every, int64_t* iters_out, double* resnorm_out,
                    void* stream) {
  if (!P || !ws || !b || !x || !state || maxiter < 0) return DSEA_ERR_ARG;
  const int64_t n = P->nloc;
  if (ws->w.n < n) return DSEA_ERR_ARG;
  if (!aligned16(b) || !aligned16(x)) return DSEA_ERR_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (poll_every <= 0) poll_every = 16;
  const bool one_reduction = (P->flags & DSEA_POP_CG_ONE_REDUCTION) ||
                             (P->kind == OP_TFIM && !(P->flags & DSEA_POP_CG_REFERENCE));
  if (one_reduction)
    return pop_cg_run_one_reduction(P, ws, shift, b, x, state, eps, maxiter, poll_every, iters_out, resnorm_out, st);
  return pop_cg_run_reference(P, ws, shift, b, x, state, eps, maxiter, poll_every, iters_out, resnorm_out, st);
}

}  // extern "C"
