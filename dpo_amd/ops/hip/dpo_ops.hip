// dpo_amd HIP/CDNA4 kernels (gfx950 / MI355X) — fp64 core math.
//
// Design notes (MI355X-first):
//  * The per-agent pose-graph problems are small (N = (d+1)n scalar rows,
//    typically 1e3..1e5; the whole working set is L2/LLC-resident), so the
//    kernels are optimized for LATENCY and FUSION, not TFLOPs: every
//    elementwise/projection pass fuses its reductions (atomicAdd into a
//    device control block) so the truncated-CG loop needs no host round
//    trips (the C++ orchestrator enqueues guarded kernels; control
//    decisions run in single-wave kernels on-device).
//  * Layout: X is (N, r) row-major fp64 ("Xt layout"): pose i occupies
//    rows [i*dh, i*dh+dh), the first d of which are the transposed
//    Stiefel block, the last the translation. Consecutive lanes read
//    consecutive (row, col) elements -> coalesced.
//  * Q is (d+1)x(d+1) block-CSR ("BSR"): row_ptr (n+1), col_idx (nnzb),
//    vals (nnzb, dh, dh). The standalone SpMM assigns a pose-block row
//    per dh*r-thread group (one output element per thread); the FUSED
//    Hessian/projection kernel computes a whole pose-block row per
//    thread with the dh x r accumulator tile in registers. fp64 FMA;
//    bandwidth/latency-bound at these sizes.
//  * Wavefront = 64; blocks are multiples of 64 threads.
//
// Functional parity targets: Hessian-vec V*Q
// (reference QuadraticProblem.cpp:68-73), tangent projection / polar
// retraction (ROPTLIB Stiefel ops), preconditioner apply
// (QuadraticProblem.cpp:75-87), G/Q assembly (PGOAgent.cpp:720-859).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

// teardown/cleanup calls whose errors are deliberately ignored
static inline void dpo_ignore(hipError_t) {}

// Debug/bisection knobs: DPO_NO_SOLVE_GRAPH=1 / DPO_NO_EVAL_GRAPH=1 run
// the solve / eval sequences eagerly instead of via cached hipGraphs.
static bool dpo_env_flag(const char* name) {
  const char* v = getenv(name);
  return v && v[0] == '1';
}

#define DPO_CHECK(x)                                                     \
  do {                                                                   \
    hipError_t _e = (x);                                                 \
    if (_e != hipSuccess) {                                              \
      fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(_e),  \
              __FILE__, __LINE__);                                       \
    }                                                                    \
  } while (0)

// ---------------------------------------------------------------------
// control block layout (fp64 slots) shared with the C++ orchestrator
// ---------------------------------------------------------------------
enum CtrlSlot {
  C_STATUS = 0,   // 0 run, 1 tcg_stop, 2 accepted, 3 give_up, 4 no_update
  C_FX = 1,
  C_GN0SQ = 2,
  C_RR = 3,
  C_ZR = 4,
  C_EPE = 5,
  C_EPD = 6,
  C_DPD = 7,
  C_COEF = 8,     // alpha or tau applied in the current eta update
  C_BETA = 9,
  C_ITER = 10,
  C_J = 11,       // snapshots stored (completed tCG iterations)
  C_RADIUS = 12,
  C_FPROP = 13,
  C_DM = 14,      // model decrease of current candidate step
  C_JSTAR = 15,
  C_TAUSTAR = 16,
  C_USE_CURRENT = 17,  // candidate step == current eta (converged tCG)
  C_STOP_PENDING = 18, // boundary/negcurv hit in current iteration
  C_BOUND = 19,        // tCG residual bound
  C_GN1SQ = 20,
  C_RHO = 21,
  C_HLEN = 22,     // valid Krylov-history entries (radius-independent)
  C_SHRINKS = 23,  // radius-shrink attempts taken (batched shrink loop)
  C_DOT0 = 24,   // scratch dot slots (cleared by ctrl kernels)
  C_DOT1 = 25,
  C_DOT2 = 26,
  C_DOT3 = 27,
  C_HIST = 32,   // 5 arrays of length MAX_TCG: z_r, d_Hd, e_Pe, e_Pd, d_Pd
};
#define MAX_TCG 16
#define H_ZR(j) (C_HIST + (j))
#define H_DHD(j) (C_HIST + MAX_TCG + (j))
#define H_EPE(j) (C_HIST + 2 * MAX_TCG + (j))
#define H_EPD(j) (C_HIST + 3 * MAX_TCG + (j))
#define H_DPD(j) (C_HIST + 4 * MAX_TCG + (j))
#define CTRL_SIZE (C_HIST + 5 * MAX_TCG)

enum Status {
  ST_RUN = 0,
  ST_TCG_STOP = 1,
  ST_ACCEPTED = 2,
  ST_GIVE_UP = 3,
  ST_NO_UPDATE = 4,
};

// guard < 0: no guard; else kernel runs only when status == guard.
__device__ __forceinline__ bool guarded_off(const double* ctrl, int guard) {
  return guard >= 0 && ctrl != nullptr && ctrl[C_STATUS] != (double)guard;
}

#define C_TICKET C_DOT3  // fan-in arrival counter (scratch slot)

// L2-coherent (L1-bypassing) ctrl accesses for the fused control tails:
// other workgroups' dot contributions arrive as device-scope atomics, so
// the last-arriving block must read them past its own L1.
__device__ __forceinline__ double ctrl_load(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ctrl_store(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Returns true for exactly one block — the last to arrive — after every
// block's prior vector-memory ops (incl. the dot atomics) have retired.
// Split-K fan-in (guide G16): per-block vmcnt drain, then a device-scope
// ticket; the winner resets the ticket for the next fused kernel. nblk is
// the number of blocks that arrive: the grid's x extent in a single-agent
// launch, the agent's own block count in a batched one.
__device__ __forceinline__ bool fanin_last_block(double* ctrl, int nblk) {
  __syncthreads();
  __shared__ int is_last;
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    double old = atomicAdd(ctrl + C_TICKET, 1.0);
    is_last = ((int)old == nblk - 1) ? 1 : 0;
    if (is_last) ctrl_store(ctrl + C_TICKET, 0.0);
  }
  __syncthreads();
  return is_last != 0;
}

// Control tails: the tCG scalar decisions, run by a single thread —
// thread 0 of the last-arriving block of the producing reduction kernel
// (fused, the default) or of a standalone k_ctrl_tail launch
// (DPO_NO_CF=1). Dot slots are read L2-coherently, results stored
// L2-visibly (the next kernel's dispatch acquire makes them visible to
// all CUs).
enum CtrlFuse { CF_NONE = 0, CF_Z0 = 1, CF_ALPHA = 2, CF_RR = 3,
                CF_BETA = 4,
                // tails of the solve head, the candidate evaluation and
                // the per-round evaluation (bodies further down)
                CF_INIT = 5, CF_ACCEPT = 6, CF_ACCEPT_OUT = 7, CF_EVAL = 8 };

// Arguments of the CF_INIT / CF_ACCEPT* / CF_EVAL tails, passed by value
// to the producing kernel (unused by the tCG tails):
//   CF_INIT        a = tol, b = Delta0, c = theta, d = kappa
//   CF_ACCEPT      a = accept_rho
//   CF_ACCEPT_OUT  a = accept_rho, dst = mapped host copy of the control
//                  block, fence = the solve's OUT fence
//   CF_EVAL        dst = the three evaluation scalars, fence = the
//                  evaluation's OUT fence (nullptr: none to release)
struct TailArgs {
  double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
  double* dst = nullptr;
  unsigned int* fence = nullptr;
};

// after z0 projection+dot (C_DOT0 = <z0, r0>)
__device__ void ctrl_tail_z0(double* ctrl) {
  if (ctrl[C_STATUS] != (double)ST_RUN) return;
  const double zr = ctrl_load(ctrl + C_DOT0);
  ctrl_store(ctrl + C_ZR, zr);
  ctrl_store(ctrl + C_DPD, zr);
  ctrl_store(ctrl + C_DOT0, 0.0);
}

// after Hd projection+dot (C_DOT0 = <delta, Hd>): alpha / boundary logic
__device__ void ctrl_tail_alpha(double* ctrl) {
  if (ctrl[C_STATUS] != (double)ST_RUN) return;
  const int j = (int)ctrl[C_ITER];
  const double d_Hd = ctrl_load(ctrl + C_DOT0);
  ctrl_store(ctrl + C_DOT0, 0.0);
  const double z_r = ctrl[C_ZR];
  const double e_Pe = ctrl[C_EPE], e_Pd = ctrl[C_EPD], d_Pd = ctrl[C_DPD];
  const double radius = ctrl[C_RADIUS];
  // scalar history for radius-replay (shrink loop reuses the Krylov path)
  ctrl_store(ctrl + H_ZR(j), z_r);
  ctrl_store(ctrl + H_DHD(j), d_Hd);
  ctrl_store(ctrl + H_EPE(j), e_Pe);
  ctrl_store(ctrl + H_EPD(j), e_Pd);
  ctrl_store(ctrl + H_DPD(j), d_Pd);
  const double alpha = z_r / d_Hd;
  const double e_Pe_new = e_Pe + 2.0 * alpha * e_Pd + alpha * alpha * d_Pd;
  if (d_Hd <= 0.0 || e_Pe_new >= radius * radius) {
    const double disc = e_Pd * e_Pd + d_Pd * (radius * radius - e_Pe);
    const double tau = (d_Pd > 0.0)
        ? (-e_Pd + sqrt(fmax(disc, 0.0))) / d_Pd : 0.0;
    ctrl_store(ctrl + C_COEF, tau);
    ctrl_store(ctrl + C_STOP_PENDING, 1.0);
  } else {
    ctrl_store(ctrl + C_COEF, alpha);
    ctrl_store(ctrl + C_EPE, e_Pe_new);
    ctrl_store(ctrl + C_STOP_PENDING, 0.0);
  }
}

// after k_tcg_update (C_DOT1 = ||r||^2 when continuing)
__device__ void ctrl_tail_rr(double* ctrl) {
  if (ctrl[C_STATUS] != (double)ST_RUN) return;
  const int j = (int)ctrl[C_ITER];
  if (ctrl[C_STOP_PENDING] != 0.0) {
    ctrl_store(ctrl + C_STATUS, (double)ST_TCG_STOP);
    ctrl_store(ctrl + C_J, (double)j);  // truncated at snapshot j
    ctrl_store(ctrl + C_HLEN, (double)(j + 1));
    ctrl_store(ctrl + C_USE_CURRENT, 0.0);
    return;
  }
  const double rr = ctrl_load(ctrl + C_DOT1);
  ctrl_store(ctrl + C_DOT1, 0.0);
  ctrl_store(ctrl + C_RR, rr);
  if (sqrt(rr) <= ctrl[C_BOUND]) {
    ctrl_store(ctrl + C_STATUS, (double)ST_TCG_STOP);
    ctrl_store(ctrl + C_J, (double)(j + 1));
    ctrl_store(ctrl + C_HLEN, (double)(j + 1));
    // converged: step = current eta
    ctrl_store(ctrl + C_USE_CURRENT, 1.0);
  }
}

// after z projection+dot (C_DOT0 = <z, r>): beta and delta scalars
__device__ void ctrl_tail_beta(double* ctrl) {
  if (ctrl[C_STATUS] != (double)ST_RUN) return;
  const double z_r_new = ctrl_load(ctrl + C_DOT0);
  ctrl_store(ctrl + C_DOT0, 0.0);
  const double z_r = ctrl[C_ZR];
  const double alpha = ctrl[C_COEF];
  const double beta = z_r_new / z_r;
  ctrl_store(ctrl + C_BETA, beta);
  ctrl_store(ctrl + C_EPD, beta * (ctrl[C_EPD] + alpha * ctrl[C_DPD]));
  ctrl_store(ctrl + C_DPD, z_r_new + beta * beta * ctrl[C_DPD]);
  ctrl_store(ctrl + C_ZR, z_r_new);
  ctrl_store(ctrl + C_ITER, ctrl[C_ITER] + 1.0);
}

// Solve head, after the gradient kernel: C_DOT0 = <QX + G, X>,
// C_DOT1 = ||grad||^2, C_DOT2 = <G, X>
//   => f = 0.5 <QX, X> + <G, X> = 0.5 (C_DOT0 + C_DOT2)
// The body of k_ctrl_init and of the CF_INIT tail.
__device__ void ctrl_body_init(double* ctrl, double tol, double Delta0,
                               double theta, double kappa) {
  const double fX = 0.5 * (ctrl_load(ctrl + C_DOT0)
                           + ctrl_load(ctrl + C_DOT2));
  const double gn0sq = ctrl_load(ctrl + C_DOT1);
  ctrl_store(ctrl + C_FX, fX);
  ctrl_store(ctrl + C_GN0SQ, gn0sq);
  ctrl_store(ctrl + C_RR, gn0sq);
  const double norm_r0 = sqrt(gn0sq);
  ctrl_store(ctrl + C_BOUND, norm_r0 * fmin(pow(norm_r0, theta), kappa));
  ctrl_store(ctrl + C_RADIUS, Delta0);
  ctrl_store(ctrl + C_EPE, 0.0);
  ctrl_store(ctrl + C_EPD, 0.0);
  ctrl_store(ctrl + C_ITER, 0.0);
  ctrl_store(ctrl + C_J, 0.0);
  ctrl_store(ctrl + C_USE_CURRENT, 0.0);
  ctrl_store(ctrl + C_STOP_PENDING, 0.0);
  ctrl_store(ctrl + C_BETA, 0.0);
  ctrl_store(ctrl + C_STATUS,
             (norm_r0 < tol) ? (double)ST_NO_UPDATE : (double)ST_RUN);
  ctrl_store(ctrl + C_DOT0, 0.0);
  ctrl_store(ctrl + C_DOT1, 0.0);
  ctrl_store(ctrl + C_DOT2, 0.0);
  ctrl_store(ctrl + C_DOT3, 0.0);
}

// Candidate selection for the current radius: replay the stored Krylov
// scalars, find the truncation point and the model decrease. The replay
// only reads (C_RADIUS, C_HLEN, the history); ctrl_candidate_store
// writes the result. The body of k_ctrl_candidate and of k_candidate.
struct CandSel {
  int jstar;  // < 0: full step (no truncation at this radius)
  double taustar, dm;
};

__device__ CandSel ctrl_candidate_replay(const double* ctrl) {
  const double radius = ctrl[C_RADIUS];
  const int hlen = (int)ctrl[C_HLEN];
  CandSel sel;
  sel.dm = 0.0;
  sel.jstar = -1;
  sel.taustar = 0.0;
  for (int j = 0; j < hlen && j < MAX_TCG; ++j) {
    const double z_r = ctrl[H_ZR(j)];
    const double d_Hd = ctrl[H_DHD(j)];
    const double e_Pe = ctrl[H_EPE(j)];
    const double e_Pd = ctrl[H_EPD(j)];
    const double d_Pd = ctrl[H_DPD(j)];
    const double alpha = z_r / d_Hd;
    const double e_Pe_new = e_Pe + 2.0 * alpha * e_Pd + alpha * alpha * d_Pd;
    if (d_Hd <= 0.0 || e_Pe_new >= radius * radius) {
      const double disc = e_Pd * e_Pd + d_Pd * (radius * radius - e_Pe);
      const double tau = (d_Pd > 0.0)
          ? (-e_Pd + sqrt(fmax(disc, 0.0))) / d_Pd : 0.0;
      sel.dm += tau * z_r - 0.5 * tau * tau * d_Hd;
      sel.jstar = j;
      sel.taustar = tau;
      break;
    }
    sel.dm += 0.5 * alpha * z_r;
  }
  return sel;
}

__device__ void ctrl_candidate_store(double* ctrl, const CandSel& sel) {
  if (sel.jstar < 0) {
    ctrl[C_USE_CURRENT] = 1.0;
  } else {
    ctrl[C_USE_CURRENT] = 0.0;
    ctrl[C_JSTAR] = (double)sel.jstar;
    ctrl[C_TAUSTAR] = sel.taustar;
  }
  ctrl[C_DM] = sel.dm;
  ctrl[C_DOT0] = 0.0;
  ctrl[C_DOT2] = 0.0;
}

// Acceptance test after the f(X_prop) dots (C_DOT0 = <QXp, Xp>,
// C_DOT2 = <G, Xp>). The body of k_ctrl_accept and of the CF_ACCEPT*
// tails.
__device__ void ctrl_body_accept(double* ctrl, double accept_rho) {
  if (ctrl[C_STATUS] != (double)ST_TCG_STOP) return;
  const double fprop = 0.5 * ctrl_load(ctrl + C_DOT0)
                       + ctrl_load(ctrl + C_DOT2);
  ctrl_store(ctrl + C_DOT0, 0.0);
  ctrl_store(ctrl + C_DOT2, 0.0);
  ctrl_store(ctrl + C_FPROP, fprop);
  const double fX = ctrl[C_FX];
  const double dm = ctrl[C_DM];
  const double rho = (fX - fprop) / fmax(dm, 1e-300);
  ctrl_store(ctrl + C_RHO, rho);
  if (rho > accept_rho && fprop <= fX) {
    ctrl_store(ctrl + C_STATUS, (double)ST_ACCEPTED);
  }
}

// Per-round evaluation, after its gradient kernel: dst[0..2] =
// [f, 0.5 <X, G>, gradnorm^2] from C_DOT0 = <QX + G, X>, C_DOT2 = <G, X>,
// C_DOT1 = ||P_X(QX + G)||^2. The dot slots are then cleaned for the
// next evaluation (solves re-zero the whole control block themselves;
// the ctx allocation is zero-initialized, so "dot slots are zero on eval
// entry" holds from the start). The body of k_eval_combine and of the
// CF_EVAL tail; the stores to dst are agent-scope because
// k_gather3_fenced reads them from another stream.
__device__ void ctrl_body_eval(double* ctrl, double* dst) {
  const double d0 = ctrl_load(ctrl + C_DOT0);
  const double d1 = ctrl_load(ctrl + C_DOT1);
  const double d2 = ctrl_load(ctrl + C_DOT2);
  ctrl_store(dst + 0, 0.5 * (d0 + d2));  // f(X)
  ctrl_store(dst + 1, 0.5 * d2);         // 0.5 <X, G>
  ctrl_store(dst + 2, d1);               // gradnorm^2
  ctrl_store(ctrl + C_DOT0, 0.0);
  ctrl_store(ctrl + C_DOT1, 0.0);
  ctrl_store(ctrl + C_DOT2, 0.0);
  ctrl_store(ctrl + C_DOT3, 0.0);
}

__device__ __forceinline__ void run_ctrl_tail(int cf, double* ctrl,
                                              const TailArgs& ta) {
  switch (cf) {
    case CF_Z0: ctrl_tail_z0(ctrl); break;
    case CF_ALPHA: ctrl_tail_alpha(ctrl); break;
    case CF_RR: ctrl_tail_rr(ctrl); break;
    case CF_BETA: ctrl_tail_beta(ctrl); break;
    case CF_INIT: ctrl_body_init(ctrl, ta.a, ta.b, ta.c, ta.d); break;
    case CF_ACCEPT:
    case CF_ACCEPT_OUT: ctrl_body_accept(ctrl, ta.a); break;
    case CF_EVAL:
      ctrl_body_eval(ctrl, ta.dst);
      // the release orders the scalars in front of the fence
      if (ta.fence)
        __hip_atomic_store(ta.fence, 1u, __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_AGENT);
      break;
    default: break;
  }
}

// End of a solve sequence, run by one whole block: copy the control
// block to the mapped host buffer, then release the solve's OUT fence.
// The system-scope fence puts every lane's host stores in front of the
// release. What k_ctrl_to_host + k_fence_signal do in two launches.
__device__ __forceinline__ void ctrl_publish(double* ctrl,
                                             const TailArgs& ta) {
  // thread 0 may just have run a tail: its stores reach L2 first
  if (threadIdx.x == 0) __threadfence();
  __syncthreads();
  for (int i = threadIdx.x; i < CTRL_SIZE; i += blockDim.x)
    ta.dst[i] = ctrl_load(ctrl + i);
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0)
    __hip_atomic_store(ta.fence, 1u, __ATOMIC_RELEASE,
                       __HIP_MEMORY_SCOPE_AGENT);
}

// wave-level + block-level reduction, then one atomicAdd per block
__device__ __forceinline__ void block_reduce_atomic(double v, double* dst) {
  __shared__ double sh[16];  // up to 1024/64 waves
  int lane = threadIdx.x & 63;
  int wave = threadIdx.x >> 6;
  for (int off = 32; off > 0; off >>= 1)
    v += __shfl_down(v, off, 64);
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  int nwaves = (blockDim.x + 63) >> 6;
  if (wave == 0) {
    double s = (lane < nwaves) ? sh[lane] : 0.0;
    for (int off = 32; off > 0; off >>= 1)
      s += __shfl_down(s, off, 64);
    if (lane == 0 && s != 0.0) atomicAdd(dst, s);
  }
  // the scratch is reused by back-to-back reductions in one kernel:
  // wave 0 must finish reading before anyone writes the next round
  __syncthreads();
}

// Epilogue of every fused reduction kernel: add this block's share of up
// to three dots into their ctrl slots (a slot < 0 is skipped; the slot
// tests are block-uniform), then — with a fused tail — fan in and let
// the last block run the control tail. A kernel that staged data through
// LDS must have put a barrier behind its last LDS read before calling.
template <int CF>
__device__ __forceinline__ void finish_reduction(double* ctrl, int nblk,
                                                 int slot0, double d0,
                                                 int slot1 = -1,
                                                 double d1 = 0.0,
                                                 int slot2 = -1,
                                                 double d2 = 0.0,
                                                 const TailArgs& ta =
                                                     TailArgs()) {
  if (slot0 >= 0) block_reduce_atomic(d0, ctrl + slot0);
  if (slot1 >= 0) block_reduce_atomic(d1, ctrl + slot1);
  if (slot2 >= 0) block_reduce_atomic(d2, ctrl + slot2);
  if (CF != CF_NONE) {
    const bool last = fanin_last_block(ctrl, nblk);
    if (last && threadIdx.x == 0) run_ctrl_tail(CF, ctrl, ta);
    if (CF == CF_ACCEPT_OUT && last) ctrl_publish(ctrl, ta);
  }
}

// ---------------------------------------------------------------------
// Per-pose building blocks shared by the kernels below. Each keeps one
// fixed order of floating-point operations, so every kernel that uses it
// produces the same bits for the same pose.
// ---------------------------------------------------------------------
// Tangent projection at X of one pose's dh x R tile held in registers:
// S = sym(Y T^T) with Y the D Stiefel rows of Xi; T -= S Y on those rows
// (the translation row is already tangent). Xi is read from memory: the
// compiler keeps the D x R values it needs in registers by itself, and
// an explicit register copy gave the same resource table.
template <int D, int R>
__device__ __forceinline__ void tangent_project(const double* Xi,
                                                double (&T)[D + 1][R]) {
  double S[D][D];
  #pragma unroll
  for (int a = 0; a < D; ++a)
    #pragma unroll
    for (int b = 0; b < D; ++b) {
      double sv = 0.0;
      #pragma unroll
      for (int k = 0; k < R; ++k) sv = fma(Xi[a * R + k], T[b][k], sv);
      S[a][b] = sv;
    }
  #pragma unroll
  for (int a = 0; a < D; ++a)
    #pragma unroll
    for (int b = a; b < D; ++b) {
      const double sv = 0.5 * (S[a][b] + S[b][a]);
      S[a][b] = sv;
      S[b][a] = sv;
    }
  #pragma unroll
  for (int a = 0; a < D; ++a)
    #pragma unroll
    for (int k = 0; k < R; ++k) {
      double v = T[a][k];
      #pragma unroll
      for (int b = 0; b < D; ++b) v = fma(-S[a][b], Xi[b * R + k], v);
      T[a][k] = v;
    }
}

// The same projection for the element-per-thread kernels: the thread
// owning element (c, k), c < D, of a pose whose X and T tiles sit in LDS
// (row-major dh x R) returns its projected value; v is its own T(c, k).
template <int D, int R>
__device__ __forceinline__ double tangent_project_lds(const double* sX,
                                                      const double* sT,
                                                      int c, int k,
                                                      double v) {
  #pragma unroll
  for (int b = 0; b < D; ++b) {
    double s1 = 0.0, s2 = 0.0;
    #pragma unroll
    for (int kk = 0; kk < R; ++kk) {
      s1 = fma(sX[c * R + kk], sT[b * R + kk], s1);
      s2 = fma(sX[b * R + kk], sT[c * R + kk], s2);
    }
    v = fma(-0.5 * (s1 + s2), sX[b * R + k], v);
  }
  return v;
}

// One column of the per-pose block-Jacobi solve L L^T y = rhs with the
// stored DH x DH Cholesky factor Li; rhs[a * stride] is row a.
template <int DH>
__device__ __forceinline__ void chol_solve_col(const double* Li,
                                               const double* rhs,
                                               size_t stride,
                                               double (&y)[DH]) {
  // forward solve L y = rhs
  #pragma unroll
  for (int a = 0; a < DH; ++a) {
    double sv = rhs[a * stride];
    #pragma unroll
    for (int b = 0; b < DH; ++b)
      if (b < a) sv = fma(-Li[a * DH + b], y[b], sv);
    y[a] = sv / Li[a * DH + a];
  }
  // backward solve L^T z = y
  #pragma unroll
  for (int a = DH - 1; a >= 0; --a) {
    double sv = y[a];
    #pragma unroll
    for (int b = 0; b < DH; ++b)
      if (b > a) sv = fma(-Li[b * DH + a], y[b], sv);
    y[a] = sv / Li[a * DH + a];
  }
}

// ---------------------------------------------------------------------
// BSR SpMM: out(N, r) = Q(N, N) @ X(N, r)
// One dh*r-thread group per pose-block row; each thread owns one
// (row_in_block, col) output element and accumulates over the row's
// blocks. Q block values are broadcast from L2 (tiny per-agent Q is
// cache-resident); X block reads are contiguous dh*r segments.
// ---------------------------------------------------------------------
template <int DH, int R>
__global__ void k_bsr_spmm(const int* __restrict__ row_ptr,
                           const int* __restrict__ col_idx,
                           const double* __restrict__ vals,
                           const double* __restrict__ X,
                           double* __restrict__ out,
                           int n, const double* __restrict__ ctrl,
                           int guard) {
  if (guarded_off(ctrl, guard)) return;
  constexpr int tile = DH * R;
  constexpr int per_block = 256 / tile;
  const int slot = threadIdx.x / tile;
  const int t = threadIdx.x % tile;
  const int i = blockIdx.x * per_block + slot;
  if (threadIdx.x >= per_block * tile || i >= n) return;
  const int c = t / R;   // row inside block
  const int k = t % R;   // column of X
  const int s = row_ptr[i], e = row_ptr[i + 1];
  double acc = 0.0;
  for (int p = s; p < e; ++p) {
    const int j = col_idx[p];
    const double* B = vals + (size_t)p * DH * DH;
    const double* Xj = X + (size_t)j * DH * R;
    #pragma unroll
    for (int cc = 0; cc < DH; ++cc)
      acc = fma(B[c * DH + cc], Xj[cc * R + k], acc);
  }
  out[(size_t)i * DH * R + c * R + k] = acc;
}

// generic-(dh, r) fallback (rare shapes); compile-time tile kernels above
__global__ void k_bsr_spmm_gen(const int* __restrict__ row_ptr,
                               const int* __restrict__ col_idx,
                               const double* __restrict__ vals,
                               const double* __restrict__ X,
                               double* __restrict__ out,
                               int n, int dh, int r,
                               const double* __restrict__ ctrl, int guard) {
  if (guarded_off(ctrl, guard)) return;
  const int tile = dh * r;
  const int per_block = blockDim.x / tile;
  const int slot = threadIdx.x / tile;
  const int t = threadIdx.x % tile;
  const int i = blockIdx.x * per_block + slot;
  if (threadIdx.x >= per_block * tile || i >= n) return;
  const int c = t / r;
  const int k = t % r;
  const int s = row_ptr[i], e = row_ptr[i + 1];
  double acc = 0.0;
  for (int p = s; p < e; ++p) {
    const int j = col_idx[p];
    const double* B = vals + (size_t)p * dh * dh;
    const double* Xj = X + (size_t)j * dh * r;
    for (int cc = 0; cc < dh; ++cc)
      acc = fma(B[c * dh + cc], Xj[cc * r + k], acc);
  }
  out[(size_t)i * dh * r + c * r + k] = acc;
}

// ---------------------------------------------------------------------
// Fused tangent projection + dots.
//   P = V (+ G) projected onto T_X; write to out.
//   Optional atomic dots: <P, dotWith> -> ctrl[dot_slot]
//                         <V+G, X> -> ctrl[dot_slot2]   (for f(X))
// One thread per pose; all of Yt (d x r), Vt (dh x r) live in registers
// (r <= DPO_MAX_R, dh <= 4).
// ---------------------------------------------------------------------
#define DPO_MAX_R 8
#define DPO_MAX_DH 4

// The kernels of the dense solve chain and of the evaluation keep their
// bodies in __device__ functions (*_body): the single-agent __global__
// kernel calls the body with its own grid extents, the batched wrapper
// (kb_*, further down) with those of the agent it serves. nblk is the
// number of blocks that take part in the kernel's fan-in.
template <int D, int R, int CF>
__device__ __forceinline__ void proj_dots_body(
    const double* __restrict__ X, const double* __restrict__ V,
    const double* __restrict__ G, double* __restrict__ out,
    const double* __restrict__ dotWith, double* __restrict__ ctrl, int n,
    int dot_slot, int dot_slot2, int guard, int nblk) {
  if (guarded_off(ctrl, guard)) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  constexpr int dh = D + 1;
  double Vt[dh][R];
  double dot_vx = 0.0;
  if (i < n) {
    const double* Xi = X + (size_t)i * dh * R;
    const double* Vi = V + (size_t)i * dh * R;
    const double* Gi = G ? G + (size_t)i * dh * R : nullptr;
    #pragma unroll
    for (int c = 0; c < dh; ++c)
      #pragma unroll
      for (int k = 0; k < R; ++k) {
        double v = Vi[c * R + k];
        if (Gi) v += Gi[c * R + k];
        Vt[c][k] = v;
        if (dot_slot2 >= 0) dot_vx = fma(v, Xi[c * R + k], dot_vx);
      }
    tangent_project<D, R>(Xi, Vt);
  }
  double dot_pw = 0.0;
  if (i < n) {
    double* Oi = out + (size_t)i * dh * R;
    const double* Wi = dotWith ? dotWith + (size_t)i * dh * R : nullptr;
    #pragma unroll
    for (int c = 0; c < dh; ++c)
      #pragma unroll
      for (int k = 0; k < R; ++k) {
        const double p = Vt[c][k];
        Oi[c * R + k] = p;
        if (dot_slot >= 0) {
          double w = Wi ? Wi[c * R + k] : p;  // default: <P,P>
          dot_pw = fma(p, w, dot_pw);
        }
      }
  }
  finish_reduction<CF>(ctrl, nblk, dot_slot, dot_pw, dot_slot2, dot_vx);
}

template <int D, int R, int CF = CF_NONE>
__global__ void k_proj_dots(const double* __restrict__ X,
                            const double* __restrict__ V,
                            const double* __restrict__ G,
                            double* __restrict__ out,
                            const double* __restrict__ dotWith,
                            double* __restrict__ ctrl,
                            int n, int dot_slot, int dot_slot2,
                            int guard) {
  proj_dots_body<D, R, CF>(X, V, G, out, dotWith, ctrl, n, dot_slot,
                           dot_slot2, guard, (int)gridDim.x);
}

// Fused block-Jacobi preconditioner apply + tangent projection (+ dot
// + control tail): one kernel instead of the {precond, proj} pair —
// one of five serial stages in every tCG iteration, so at large N the
// removed launch+drain latency is pure win. Per pose: y = M^-1 r via
// the cached per-pose Cholesky factors, P = P_X(y), dot <P, r>.
template <int D, int R, int CF = CF_NONE>
__global__ void k_precond_proj(const double* __restrict__ L,
                               const double* __restrict__ rvec,
                               const double* __restrict__ X,
                               double* __restrict__ Z,
                               double* __restrict__ ctrl,
                               int n, int dot_slot, int guard) {
  if (guarded_off(ctrl, guard)) return;
  constexpr int dh = D + 1;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double Vt[dh][R];
  double dot = 0.0;
  if (i < n) {
    const double* Li = L + (size_t)i * dh * dh;
    const double* Ri = rvec + (size_t)i * dh * R;
    // chol_solve_col and tangent_project written out, same operation
    // order: through the helpers this kernel alone compiles to a
    // different schedule (d = 3, r = 5: 92 instead of 114 VGPRs, fewer
    // loads in flight) that measured 2.5-3.5 % slower per 1M-pose round.
    #pragma unroll
    for (int k = 0; k < R; ++k) {
      double y[dh];
      #pragma unroll
      for (int a = 0; a < dh; ++a) {
        double sv = Ri[a * R + k];
        #pragma unroll
        for (int b = 0; b < dh; ++b)
          if (b < a) sv = fma(-Li[a * dh + b], y[b], sv);
        y[a] = sv / Li[a * dh + a];
      }
      #pragma unroll
      for (int a = dh - 1; a >= 0; --a) {
        double sv = y[a];
        #pragma unroll
        for (int b = 0; b < dh; ++b)
          if (b > a) sv = fma(-Li[b * dh + a], y[b], sv);
        y[a] = sv / Li[a * dh + a];
      }
      #pragma unroll
      for (int a = 0; a < dh; ++a) Vt[a][k] = y[a];
    }
    const double* Xi = X + (size_t)i * dh * R;
    double S[D][D];
    #pragma unroll
    for (int a = 0; a < D; ++a)
      #pragma unroll
      for (int b = 0; b < D; ++b) {
        double sv = 0.0;
        #pragma unroll
        for (int k = 0; k < R; ++k)
          sv = fma(Xi[a * R + k], Vt[b][k], sv);
        S[a][b] = sv;
      }
    #pragma unroll
    for (int a = 0; a < D; ++a)
      #pragma unroll
      for (int b = a; b < D; ++b) {
        const double sv = 0.5 * (S[a][b] + S[b][a]);
        S[a][b] = sv;
        S[b][a] = sv;
      }
    #pragma unroll
    for (int a = 0; a < D; ++a)
      #pragma unroll
      for (int k = 0; k < R; ++k) {
        double v = Vt[a][k];
        #pragma unroll
        for (int b = 0; b < D; ++b) v = fma(-S[a][b], Xi[b * R + k], v);
        Vt[a][k] = v;
      }
    double* Zi = Z + (size_t)i * dh * R;
    #pragma unroll
    for (int c = 0; c < dh; ++c)
      #pragma unroll
      for (int k = 0; k < R; ++k) {
        Zi[c * R + k] = Vt[c][k];
        if (dot_slot >= 0)
          dot = fma(Vt[c][k], Ri[c * R + k], dot);
      }
  }
  finish_reduction<CF>(ctrl, gridDim.x, dot_slot, dot);
}

// Wide (element-per-thread) tangent projection for LARGE agents: same
// wave-starvation fix as k_hess_wide (a thread-per-pose kernel gets
// only n/64 waves). dh*r threads per pose; the cross-element sym(Y V^T)
// contraction goes through LDS tiles.
template <int D, int R, int CF = CF_NONE>
__global__ void k_proj_wide(const double* __restrict__ X,
                            const double* __restrict__ V,
                            const double* __restrict__ G,
                            double* __restrict__ out,
                            const double* __restrict__ dotWith,
                            double* __restrict__ ctrl,
                            int n, int dot_slot, int dot_slot2,
                            int guard) {
  if (guarded_off(ctrl, guard)) return;
  constexpr int dh = D + 1;
  constexpr int TILE = dh * R;
  constexpr int PB = 256 / TILE;
  __shared__ double sV[PB][TILE];
  __shared__ double sX[PB][TILE];
  const int slot = threadIdx.x / TILE;
  const int e = threadIdx.x % TILE;
  const int c = e / R;
  const int k = e % R;
  const bool active = threadIdx.x < PB * TILE;
  const int i = blockIdx.x * PB + slot;
  const bool live = active && i < n;
  double v = 0.0, x = 0.0, d0 = 0.0, d1 = 0.0;
  if (live) {
    v = V[(size_t)i * TILE + e];
    if (G) v += G[(size_t)i * TILE + e];
    x = X[(size_t)i * TILE + e];
    if (dot_slot2 >= 0) d1 = v * x;
    sV[slot][e] = v;
    sX[slot][e] = x;
  }
  __syncthreads();
  double o = v;
  if (live && c < D)
    o = tangent_project_lds<D, R>(sX[slot], sV[slot], c, k, v);
  if (live) {
    out[(size_t)i * TILE + e] = o;
    if (dot_slot >= 0) {
      const double w = dotWith ? dotWith[(size_t)i * TILE + e] : o;
      d0 = o * w;
    }
  }
  __syncthreads();
  finish_reduction<CF>(ctrl, gridDim.x, dot_slot, d0, dot_slot2, d1);
}

// ---------------------------------------------------------------------
// Fused Hessian-vector product: one THREAD per pose computes its whole
// BSR row of Q @ V (the dh x r accumulator tile lives in registers; each
// Q block is one 128-byte line), optionally adds G, applies the tangent
// projection at X, writes the result and accumulates the requested dot
// products — replacing a {SpMM kernel, projection kernel} pair with one
// launch. MODE 0: out = P_X(QV + G), dots <out, dotW> / <QV+G, X>.
// MODE 1 (no projection, no store): dots <QV, V> and <G, V> (the
// trust-region candidate's f evaluation).
// ---------------------------------------------------------------------
// AUX = 1 (MODE 0 only) adds two optional side effects for the solve's
// gradient launch: a second copy of the result in out2, and zero_out's
// rows of this pose cleared. A template parameter, so that the tCG-loop
// instantiations keep their register budget.
// AUX = 2 (MODE 0 only) is the tCG Hd stage with the direction update
// folded in: the direction delta = beta * delta_old - z is not read from
// memory but formed per neighbour as fma(beta, delta_old[j], -z[j]), the
// single fma of k_tcg_delta, so the bits are the same. delta is double
// buffered (zero_out = buffer 0, out2 = buffer 1, dotW = z; V is not
// used): iteration C_ITER
// writes its own pose's tile into buffer C_ITER & 1 and reads the other,
// so no block reads what another writes, and the choice travels with the
// control block across the continuation graph.
template <int D, int R, int MODE, int CF, int AUX>
__device__ __forceinline__ void hess_fused_body(
    const int* __restrict__ row_ptr, const int* __restrict__ col_idx,
    const double* __restrict__ vals, const double* __restrict__ V,
    const double* __restrict__ X, const double* __restrict__ G,
    double* __restrict__ out, const double* __restrict__ dotW,
    double* __restrict__ ctrl, int n, int dot_slot, int dot_slot2,
    int dot_slot3, int guard, double* __restrict__ out2,
    double* __restrict__ zero_out, TailArgs ta, int nblk) {
  if (guarded_off(ctrl, guard)) {
    // the CF_ACCEPT_OUT publish step is unguarded, like the two launches
    // it replaces: the host reads the control block whatever the status
    if (CF == CF_ACCEPT_OUT && blockIdx.x == 0) ctrl_publish(ctrl, ta);
    return;
  }
  constexpr int dh = D + 1;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double acc[dh][R];
  double d0 = 0.0, d1 = 0.0, d2 = 0.0;
  // AUX == 2: old / new direction buffer by the parity of C_ITER
  const double* dold = nullptr;
  double* dnew = nullptr;
  double beta = 0.0;
  if (AUX == 2) {
    const bool odd = ((int)ctrl[C_ITER]) & 1;
    dold = odd ? zero_out : out2;
    dnew = odd ? out2 : zero_out;
    beta = ctrl[C_BETA];
  }
  if (i < n) {
    #pragma unroll
    for (int c = 0; c < dh; ++c)
      #pragma unroll
      for (int k = 0; k < R; ++k) acc[c][k] = 0.0;
    const int s0 = row_ptr[i], e0 = row_ptr[i + 1];
    for (int p = s0; p < e0; ++p) {
      const double* B = vals + (size_t)p * dh * dh;
      const size_t jo = (size_t)col_idx[p] * dh * R;
      if (AUX == 2) {
        // one row of the neighbour's direction at a time (R values live
        // instead of the tile); every acc[c][k] still adds its cc terms
        // in the order 0 .. dh-1, as below
        #pragma unroll
        for (int cc = 0; cc < dh; ++cc) {
          double v[R];
          #pragma unroll
          for (int k = 0; k < R; ++k)
            v[k] = fma(beta, dold[jo + cc * R + k], -dotW[jo + cc * R + k]);
          #pragma unroll
          for (int c = 0; c < dh; ++c) {
            const double b = B[c * dh + cc];
            #pragma unroll
            for (int k = 0; k < R; ++k) acc[c][k] = fma(b, v[k], acc[c][k]);
          }
          // keep the next rows' loads from being hoisted over this one
          __builtin_amdgcn_sched_barrier(0);
        }
        continue;
      }
      const double* Vj = V + jo;
      #pragma unroll
      for (int c = 0; c < dh; ++c)
        #pragma unroll
        for (int cc = 0; cc < dh; ++cc) {
          const double b = B[c * dh + cc];
          #pragma unroll
          for (int k = 0; k < R; ++k)
            acc[c][k] = fma(b, Vj[cc * R + k], acc[c][k]);
        }
    }
    if (G) {
      const double* Gi = G + (size_t)i * dh * R;
      const double* Xi3 = (MODE == 0 && dot_slot3 >= 0)
          ? X + (size_t)i * dh * R : nullptr;
      #pragma unroll
      for (int c = 0; c < dh; ++c)
        #pragma unroll
        for (int k = 0; k < R; ++k) {
          const double g = Gi[c * R + k];
          acc[c][k] += g;
          if (Xi3) d2 = fma(g, Xi3[c * R + k], d2);
        }
    }
    if (MODE == 1) {
      // dots only: d0 = <(QV)_i + G_i, V_i>, d1 = <G_i, V_i>
      const double* Vi = V + (size_t)i * dh * R;
      const double* Gi = G ? G + (size_t)i * dh * R : nullptr;
      #pragma unroll
      for (int c = 0; c < dh; ++c)
        #pragma unroll
        for (int k = 0; k < R; ++k) {
          const double g = Gi ? Gi[c * R + k] : 0.0;
          d0 = fma(acc[c][k] - g, Vi[c * R + k], d0);
          d1 = fma(g, Vi[c * R + k], d1);
        }
    } else {
      const double* Xi = X + (size_t)i * dh * R;
      if (dot_slot2 >= 0) {
        #pragma unroll
        for (int c = 0; c < dh; ++c)
          #pragma unroll
          for (int k = 0; k < R; ++k)
            d1 = fma(acc[c][k], Xi[c * R + k], d1);
      }
      tangent_project<D, R>(Xi, acc);
      double* Oi = out + (size_t)i * dh * R;
      double* O2 = (AUX == 1 && out2) ? out2 + (size_t)i * dh * R : nullptr;
      const double* Wi = dotW ? dotW + (size_t)i * dh * R : nullptr;
      #pragma unroll
      for (int c = 0; c < dh; ++c)
        #pragma unroll
        for (int k = 0; k < R; ++k) {
          Oi[c * R + k] = acc[c][k];
          if (AUX == 1 && O2) O2[c * R + k] = acc[c][k];
          if (AUX != 2 && dot_slot >= 0) {
            const double w = Wi ? Wi[c * R + k] : acc[c][k];
            d0 = fma(acc[c][k], w, d0);
          }
        }
      if (AUX == 2) {
        // this pose's tile of the new direction and <delta, Hd>, in a
        // pass of its own behind the projection so that its loads are
        // not live across it; same element order as the loop above
        __builtin_amdgcn_sched_barrier(0);
        #pragma unroll
        for (int c = 0; c < dh; ++c)
          #pragma unroll
          for (int k = 0; k < R; ++k) {
            const size_t e = (size_t)i * dh * R + c * R + k;
            const double w = fma(beta, dold[e], -dotW[e]);
            dnew[e] = w;
            d0 = fma(acc[c][k], w, d0);
          }
      }
      // clears the buffer in front of the next dense apply
      if (AUX == 1 && zero_out) {
        double* Zi = zero_out + (size_t)i * dh * R;
        #pragma unroll
        for (int e = 0; e < dh * R; ++e) Zi[e] = 0.0;
      }
    }
  }
  finish_reduction<CF>(ctrl, nblk, dot_slot, d0, dot_slot2, d1,
                       MODE == 0 ? dot_slot3 : -1, d2, ta);
}

template <int D, int R, int MODE, int CF = CF_NONE, int AUX = 0>
__global__ void k_hess_fused(const int* __restrict__ row_ptr,
                             const int* __restrict__ col_idx,
                             const double* __restrict__ vals,
                             const double* __restrict__ V,
                             const double* __restrict__ X,
                             const double* __restrict__ G,
                             double* __restrict__ out,
                             const double* __restrict__ dotW,
                             double* __restrict__ ctrl,
                             int n, int dot_slot, int dot_slot2,
                             int dot_slot3, int guard,
                             double* __restrict__ out2,
                             double* __restrict__ zero_out, TailArgs ta) {
  hess_fused_body<D, R, MODE, CF, AUX>(row_ptr, col_idx, vals, V, X, G, out,
                                       dotW, ctrl, n, dot_slot, dot_slot2,
                                       dot_slot3, guard, out2, zero_out, ta,
                                       (int)gridDim.x);
}

// ---------------------------------------------------------------------
// Wide (element-per-thread) variant of k_hess_fused for LARGE agents.
// One thread per pose-tile ELEMENT (dh*r threads per pose, 256/tile
// poses per block): a 125k-pose agent then launches ~39k waves instead
// of the ~2k a thread-per-pose kernel gets (which is < 2 waves/SIMD on
// 256 CUs — too few to hide HBM latency, the round-1 1M-pose
// bottleneck). The SpMM phase reads each neighbor block cooperatively;
// the cross-element tangent projection stages the acc tile and X tile
// through LDS. Same math and dot-product contract as k_hess_fused.
// ---------------------------------------------------------------------
template <int D, int R, int MODE, int CF = CF_NONE, int AUX = 0>
__global__ void k_hess_wide(const int* __restrict__ row_ptr,
                            const int* __restrict__ col_idx,
                            const double* __restrict__ vals,
                            const double* __restrict__ V,
                            const double* __restrict__ X,
                            const double* __restrict__ G,
                            double* __restrict__ out,
                            const double* __restrict__ dotW,
                            double* __restrict__ ctrl,
                            int n, int dot_slot, int dot_slot2,
                            int dot_slot3, int guard,
                            double* __restrict__ out2,
                            double* __restrict__ zero_out, TailArgs ta) {
  if (guarded_off(ctrl, guard)) {
    // the CF_ACCEPT_OUT publish step is unguarded, like the two launches
    // it replaces: the host reads the control block whatever the status
    if (CF == CF_ACCEPT_OUT && blockIdx.x == 0) ctrl_publish(ctrl, ta);
    return;
  }
  constexpr int dh = D + 1;
  constexpr int TILE = dh * R;
  constexpr int PB = 256 / TILE;  // poses per block
  __shared__ double sAcc[PB][TILE];
  __shared__ double sX[PB][TILE];
  const int slot = threadIdx.x / TILE;
  const int e = threadIdx.x % TILE;
  const int c = e / R;            // row inside the dh x R tile
  const int k = e % R;            // column
  const bool active = threadIdx.x < PB * TILE;
  const int i = blockIdx.x * PB + slot;
  const bool live = active && i < n;
  double acc = 0.0;
  double d0 = 0.0, d1 = 0.0, d2 = 0.0;
  if (live) {
    const int s0 = row_ptr[i], e0 = row_ptr[i + 1];
    for (int p = s0; p < e0; ++p) {
      const int j = col_idx[p];            // uniform across the tile
      const double* B = vals + (size_t)p * dh * dh + c * dh;
      const double* Vj = V + (size_t)j * dh * R + k;
      #pragma unroll
      for (int cc = 0; cc < dh; ++cc)
        acc = fma(B[cc], Vj[cc * R], acc);
    }
    const double g = G ? G[(size_t)i * TILE + e] : 0.0;
    acc += g;
    if (MODE == 0 && dot_slot3 >= 0 && G)
      d2 = g * X[(size_t)i * TILE + e];
    if (MODE == 1) {
      const double v = V[(size_t)i * TILE + e];
      d0 = (acc - g) * v;
      d1 = g * v;
    } else {
      const double x = X[(size_t)i * TILE + e];
      if (dot_slot2 >= 0) d1 = acc * x;
      sAcc[slot][e] = acc;
      sX[slot][e] = x;
    }
  }
  if (MODE == 0) {
    __syncthreads();
    double o = acc;
    if (live && c < D)
      o = tangent_project_lds<D, R>(sX[slot], sAcc[slot], c, k, acc);
    if (live) {
      out[(size_t)i * TILE + e] = o;
      if (AUX && out2) out2[(size_t)i * TILE + e] = o;
      if (AUX && zero_out) zero_out[(size_t)i * TILE + e] = 0.0;
      if (dot_slot >= 0) {
        const double w = dotW ? dotW[(size_t)i * TILE + e] : o;
        d0 = o * w;
      }
    }
    __syncthreads();  // sAcc/sX reuse barrier for CF tail safety
  }
  finish_reduction<CF>(ctrl, gridDim.x, dot_slot, d0, dot_slot2, d1,
                       MODE == 0 ? dot_slot3 : -1, d2, ta);
}

// ---------------------------------------------------------------------
// fp64-MFMA BSR SpMM (A/B study, round-1 VERDICT item 4; d = 3 only).
// One wave computes 4 pose rows as a 16x16 v_mfma_f64_16x16x4_f64 tile
// accumulating over the 4-row group's COLUMN UNION (grouped-ELL built
// host-side): A = the 4 poses' stacked 4x4 Q blocks for union column u
// (zeros where a pose lacks that column), B = the neighbor pose block
// V_j (cols 5..15 zero-padded). Useful-FLOP ratio is r/16 x the union
// fill (~20-30% at r=5), and gfx950's fp64 matrix rate equals the
// vector rate, so this is expected to LOSE to the scalar-FMA kernels —
// the point is to measure that, with rocprof counters, instead of
// arguing it.
// ---------------------------------------------------------------------
typedef double dpo_d4 __attribute__((ext_vector_type(4)));

__global__ void k_bsr_spmm_mfma_d3(const int* __restrict__ grp_ptr,
                                   const int* __restrict__ grp_cols,
                                   const int* __restrict__ grp_blk,
                                   const double* __restrict__ vals,
                                   const double* __restrict__ X,
                                   double* __restrict__ out,
                                   int ngroups, int n, int r) {
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * (blockDim.x >> 6) + wave;
  if (g >= ngroups) return;
  const int row16 = lane & 15;        // A row: pose-in-group*4 + brow
  const int kfrag = lane >> 4;        // K index 0..3
  const int pose_in_g = row16 >> 2;
  const int brow = row16 & 3;
  dpo_d4 acc = {0.0, 0.0, 0.0, 0.0};
  const int s0 = grp_ptr[g], e0 = grp_ptr[g + 1];
  for (int u = s0; u < e0; ++u) {
    const int j = grp_cols[u];
    const int blk = grp_blk[(size_t)u * 4 + pose_in_g];
    const double a = (blk >= 0)
        ? vals[(size_t)blk * 16 + brow * 4 + kfrag] : 0.0;
    const int col = lane & 15;
    const double b = (col < r)
        ? X[(size_t)j * 4 * r + kfrag * r + col] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
  // D layout (probed on gfx950, scripts/mfma_probe.py): lane l, reg q
  // -> D[row = 4*q + (l>>4)][col = l&15]
  const int col = lane & 15;
  if (col < r) {
    #pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = 4 * q + (lane >> 4);
      const int pose = g * 4 + (row >> 2);
      if (pose < n)
        out[(size_t)pose * 4 * r + (row & 3) * r + col] = acc[q];
    }
  }
}

// ---------------------------------------------------------------------
// Batched polar projection onto (St(d, r) x R^r)^n of an affine
// combination  M = ca*A + cb*B + cc*C  (B, C optional).
// polar(Mt) for the wide d x r Stiefel block via the analytic
// eigendecomposition of the d x d Gram matrix (d <= 3).
// Translations pass through the affine combination unchanged.
// One thread per pose, everything in registers.
// ---------------------------------------------------------------------
// Inverse square root of a d x d SPD Gram matrix via the coupled
// Newton-Schulz iteration (trace-scaled):  Y -> A^{1/2}, Z -> A^{-1/2}.
// Branch-free and exact in the fully-degenerate case (Gram ~ c*I), which
// is the common case for retractions (X + small step is near-Stiefel) —
// an analytic eigenvector decomposition is ill-conditioned exactly there.
template <int D>
__device__ __forceinline__ void spd_inv_sqrt(const double S[D][D],
                                             double out[D][D]) {
  double tr = 0.0;
  #pragma unroll
  for (int i = 0; i < D; ++i) tr += S[i][i];
  if (tr <= 1e-300) {
    #pragma unroll
    for (int i = 0; i < D; ++i)
      #pragma unroll
      for (int j = 0; j < D; ++j) out[i][j] = 0.0;
    return;
  }
  const double inv_s = 1.0 / tr;
  double Y[D][D], Z[D][D];
  #pragma unroll
  for (int i = 0; i < D; ++i)
    #pragma unroll
    for (int j = 0; j < D; ++j) {
      Y[i][j] = S[i][j] * inv_s;
      Z[i][j] = (i == j) ? 1.0 : 0.0;
    }
  for (int it = 0; it < 40; ++it) {
    // T = (3 I - Z Y) / 2
    double T[D][D];
    double delta = 0.0;
    #pragma unroll
    for (int i = 0; i < D; ++i)
      #pragma unroll
      for (int j = 0; j < D; ++j) {
        double acc = 0.0;
        #pragma unroll
        for (int k = 0; k < D; ++k) acc = fma(Z[i][k], Y[k][j], acc);
        T[i][j] = 0.5 * (((i == j) ? 3.0 : 0.0) - acc);
        const double dij = T[i][j] - ((i == j) ? 1.0 : 0.0);
        delta += dij * dij;
      }
    double Yn[D][D], Zn[D][D];
    #pragma unroll
    for (int i = 0; i < D; ++i)
      #pragma unroll
      for (int j = 0; j < D; ++j) {
        double ay = 0.0, az = 0.0;
        #pragma unroll
        for (int k = 0; k < D; ++k) {
          ay = fma(Y[i][k], T[k][j], ay);
          az = fma(T[i][k], Z[k][j], az);
        }
        Yn[i][j] = ay;
        Zn[i][j] = az;
      }
    #pragma unroll
    for (int i = 0; i < D; ++i)
      #pragma unroll
      for (int j = 0; j < D; ++j) {
        Y[i][j] = Yn[i][j];
        Z[i][j] = Zn[i][j];
      }
    if (delta < 1e-30) break;  // converged (T ~ I)
  }
  const double c = rsqrt(tr);
  #pragma unroll
  for (int i = 0; i < D; ++i)
    #pragma unroll
    for (int j = 0; j < D; ++j) out[i][j] = Z[i][j] * c;
}

// Oi = one pose's polar projection of the register tile Mt: polar of its
// D Stiefel rows, the translation row unchanged.
template <int D, int R>
__device__ __forceinline__ void polar_tile(const double (&Mt)[D + 1][R],
                                           double* Oi) {
  // Gram = Mt Mt^T (D x D); polar(Mt) = Gram^{-1/2} Mt
  double S[D][D];
  #pragma unroll
  for (int a = 0; a < D; ++a)
    #pragma unroll
    for (int b = 0; b < D; ++b) {
      double s = 0.0;
      #pragma unroll
      for (int k = 0; k < R; ++k) s = fma(Mt[a][k], Mt[b][k], s);
      S[a][b] = s;
    }
  double Gi[D][D];
  spd_inv_sqrt<D>(S, Gi);
  #pragma unroll
  for (int a = 0; a < D; ++a)
    #pragma unroll
    for (int k = 0; k < R; ++k) {
      double s = 0.0;
      #pragma unroll
      for (int b = 0; b < D; ++b) s = fma(Gi[a][b], Mt[b][k], s);
      Oi[a * R + k] = s;
    }
  #pragma unroll
  for (int k = 0; k < R; ++k) Oi[D * R + k] = Mt[D][k];
}

template <int D, int R>
__global__ void k_polar_affine(const double* __restrict__ A,
                               const double* __restrict__ B,
                               const double* __restrict__ C,
                               double ca, double cb, double cc,
                               double* __restrict__ out,
                               int n, const double* __restrict__ ctrl,
                               int guard) {
  if (guarded_off(ctrl, guard)) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int dh = D + 1;
  double Mt[dh][R];
  const double* Ai = A + (size_t)i * dh * R;
  const double* Bi = B ? B + (size_t)i * dh * R : nullptr;
  const double* Ci = C ? C + (size_t)i * dh * R : nullptr;
  #pragma unroll
  for (int c = 0; c < dh; ++c)
    #pragma unroll
    for (int k = 0; k < R; ++k) {
      double v = ca * Ai[c * R + k];
      if (Bi) v = fma(cb, Bi[c * R + k], v);
      if (Ci) v = fma(cc, Ci[c * R + k], v);
      Mt[c][k] = v;
    }
  polar_tile<D, R>(Mt, out + (size_t)i * dh * R);
}

// ---------------------------------------------------------------------
// Dense fp32 preconditioner apply: Z(N, r) = Minv(N, N) @ V(N, r).
// Minv is symmetric -> read as Minv[j*N+i], so the lanes that share a
// matrix row j read consecutive output rows i (coalesced).
// fp32 storage halves the bandwidth; accumulate fp64.
// ---------------------------------------------------------------------
// A block owns a strip of DENSE_STRIP output rows, one 128-byte segment
// of every matrix row, and the whole j range: no sum crosses a block, so
// Z is written with plain stores in a fixed summation order (no atomics,
// no zeroed output, bit-reproducible). Eight lanes cover a row's segment
// with four output rows each; a wave takes 8 matrix rows per load
// instruction and the 256-thread block DENSE_ROWS = 32. Every lane keeps
// DENSE_LOADS independent loads in flight before the first is consumed,
// so V is staged through LDS in tiles of 32 * DENSE_LOADS rows.
constexpr int DENSE_STRIP = 32;
constexpr int DENSE_ROWS = 32;
constexpr int DENSE_LOADS = 8;
constexpr int DENSE_TILE_J = DENSE_ROWS * DENSE_LOADS;

static inline int precond_dense_strips(int N) {
  return (N + DENSE_STRIP - 1) / DENSE_STRIP;
}

// The 16-byte loads need every row segment aligned: N % 4 == 0 and an
// aligned base (every d = 3 shape). Anything else takes the VEC = false
// instantiation: 4-byte loads, the same strip, reduction and stores, and
// therefore the same bits.
static inline bool precond_dense_vec_ok(const float* Minv, int N) {
  return N % 4 == 0 && ((uintptr_t)Minv & 15) == 0;
}

// One lane's loads of a tile of DENSE_TILE_J matrix rows from j0: its
// DENSE_LOADS pieces of four matrix entries and its R elements of the V
// tile. Branch-free and unmasked, so every load is in flight and nothing
// waits here: addresses are clamped into the arrays (a row at or beyond N
// re-reads the last one), and the consumer zeroes the V tile's rows at or
// beyond N instead.
template <int R>
struct DenseTile {
  float m[DENSE_LOADS][4];
  double v[R];
};

template <int R, bool VEC>
__device__ __forceinline__ void dense_tile_load(
    DenseTile<R>& t, const float* __restrict__ Minv,
    const double* __restrict__ V, int N, int j0, int i) {
  const int tid = threadIdx.x;
  const int g = tid >> 3;
  #pragma unroll
  for (int u = 0; u < DENSE_LOADS; ++u) {
    const int j = j0 + g + DENSE_ROWS * u;
    const float* Mj = Minv + (size_t)min(j, N - 1) * N;
    if (VEC) {
      const float4 f = *reinterpret_cast<const float4*>(Mj + (i < N ? i : 0));
      t.m[u][0] = f.x; t.m[u][1] = f.y; t.m[u][2] = f.z; t.m[u][3] = f.w;
    } else {
      #pragma unroll
      for (int v = 0; v < 4; ++v) t.m[u][v] = Mj[min(i + v, N - 1)];
    }
  }
  const long total = (long)N * R;
  #pragma unroll
  for (int c = 0; c < R; ++c) {
    const long e = (long)j0 * R + tid + 256 * c;
    t.v[c] = V[e < total ? e : total - 1];
  }
}

// Element `threadIdx.x` of the strip's DENSE_STRIP x R block of Z (row-
// major, contiguous in Z), valid in threads < DENSE_STRIP * R; sh holds
// DENSE_TILE_J * R doubles. Rows at or beyond N come out as zero. Every
// thread of the 256-thread block must call it (barriers inside).
template <int R, bool VEC>
__device__ __forceinline__ double precond_dense_strip_sum(
    const float* __restrict__ Minv, const double* __restrict__ V, int N,
    int strip, double* sh) {
  static_assert(DENSE_STRIP * R <= 256 && 4 * DENSE_STRIP <= DENSE_TILE_J,
                "strip tile must fit the block and the V tile");
  const int tid = threadIdx.x;
  const int q = tid & 7;   // which 4 output rows of the strip
  const int g = tid >> 3;  // which matrix row of a pass of DENSE_ROWS
  const int i = strip * DENSE_STRIP + 4 * q;
  double acc[4][R];
  #pragma unroll
  for (int v = 0; v < 4; ++v)
    #pragma unroll
    for (int k = 0; k < R; ++k) acc[v][k] = 0.0;
  // The next tile's loads are issued behind the barriers and in front of
  // the current tile's arithmetic, which hides their round trip; the
  // scheduling barrier keeps the compiler from sinking them below it.
  const long total = (long)N * R;
  DenseTile<R> nxt;
  dense_tile_load<R, VEC>(nxt, Minv, V, N, 0, i);
  for (int j0 = 0; j0 < N; j0 += DENSE_TILE_J) {
    const DenseTile<R> cur = nxt;
    __syncthreads();
    #pragma unroll
    for (int c = 0; c < R; ++c)
      sh[tid + 256 * c] =
          (long)j0 * R + tid + 256 * c < total ? cur.v[c] : 0.0;
    __syncthreads();
    dense_tile_load<R, VEC>(nxt, Minv, V, N, j0 + DENSE_TILE_J, i);
    __builtin_amdgcn_sched_barrier(0);
    #pragma unroll
    for (int u = 0; u < DENSE_LOADS; ++u)
      #pragma unroll
      for (int k = 0; k < R; ++k) {
        const double vk = sh[(g + DENSE_ROWS * u) * R + k];
        #pragma unroll
        for (int v = 0; v < 4; ++v)
          acc[v][k] = fma((double)cur.m[u][v], vk, acc[v][k]);
      }
  }
  // the wave's 8 row groups in a fixed butterfly order, then the 4 waves
  // through LDS in a fixed order
  #pragma unroll
  for (int v = 0; v < 4; ++v)
    #pragma unroll
    for (int k = 0; k < R; ++k) {
      double s = acc[v][k];
      s += __shfl_xor(s, 8);
      s += __shfl_xor(s, 16);
      s += __shfl_xor(s, 32);
      acc[v][k] = s;
    }
  __syncthreads();
  if ((tid & 63) < 8) {
    double* dst = sh + ((tid >> 6) * DENSE_STRIP + 4 * q) * R;
    #pragma unroll
    for (int v = 0; v < 4; ++v)
      #pragma unroll
      for (int k = 0; k < R; ++k) dst[v * R + k] = acc[v][k];
  }
  __syncthreads();
  constexpr int SR = DENSE_STRIP * R;
  double zt = 0.0;
  if (tid < SR)
    zt = ((sh[tid] + sh[SR + tid]) + sh[2 * SR + tid]) + sh[3 * SR + tid];
  return zt;
}

template <int R, bool VEC>
__device__ __forceinline__ void precond_dense_body(
    const float* __restrict__ Minv, const double* __restrict__ V,
    double* __restrict__ Z, int N, const double* __restrict__ ctrl,
    int guard, int strip) {
  if (guarded_off(ctrl, guard)) return;
  __shared__ double sh[DENSE_TILE_J * R];
  const double zt = precond_dense_strip_sum<R, VEC>(Minv, V, N, strip, sh);
  const long e = (long)strip * DENSE_STRIP * R + threadIdx.x;
  if ((int)threadIdx.x < DENSE_STRIP * R && e < (long)N * R) Z[e] = zt;
}

template <int R, bool VEC>
__global__ void __launch_bounds__(256)
k_precond_dense(const float* __restrict__ Minv, const double* __restrict__ V,
                double* __restrict__ Z, int N,
                const double* __restrict__ ctrl, int guard) {
  precond_dense_body<R, VEC>(Minv, V, Z, N, ctrl, guard, (int)blockIdx.x);
}

// Block-Jacobi apply: per pose solve (L L^T) z = v with stored Cholesky
// factors L (n, dh, dh). One thread per pose per rhs column.
template <int DH>
__global__ void k_precond_jacobi(const double* __restrict__ L,
                                 const double* __restrict__ V,
                                 double* __restrict__ Z,
                                 int n, int r,
                                 const double* __restrict__ ctrl, int guard) {
  if (guarded_off(ctrl, guard)) return;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * r) return;
  const int i = idx / r, k = idx % r;
  double y[DH];
  chol_solve_col<DH>(L + (size_t)i * DH * DH, V + (size_t)i * DH * r + k, r,
                     y);
  #pragma unroll
  for (int a = 0; a < DH; ++a) Z[((size_t)i * DH + a) * r + k] = y[a];
}

// ---------------------------------------------------------------------
// Fused tCG vector updates (guarded; coefficients read from ctrl):
//   snapshot: eta_snap[j] = eta, delta_snap[j] = delta  (pre-update)
//   eta += coef * delta;  if (!stop_pending) { r += alpha*Hd; rr+=r^2 }
//   zero_out (optional) = 0
// ---------------------------------------------------------------------
// Two elements per thread: the kernel is a pure fp64 stream (4 reads
// + 4 writes per element) and was memory-latency-bound at 1M-pose
// scale with one 8-byte access per lane per array.
template <int CF>
__device__ __forceinline__ void tcg_update_body(
    double* __restrict__ eta, double* __restrict__ rvec,
    const double* __restrict__ delta0, const double* __restrict__ Hd,
    double* __restrict__ eta_snap, double* __restrict__ delta_snap,
    double* __restrict__ ctrl, long total, double* __restrict__ zero_out,
    const double* __restrict__ delta1, int nblk) {
  if (guarded_off(ctrl, ST_RUN)) return;
  const long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const double coef = ctrl[C_COEF];
  const int stop_pending = (int)ctrl[C_STOP_PENDING];
  const int j = (int)ctrl[C_ITER];
  // double-buffered direction (delta1 != nullptr): iteration j's lives
  // in buffer j & 1, where the Hd stage in front wrote it
  const double* delta = (delta1 && (j & 1)) ? delta1 : delta0;
  double rr = 0.0;
  #pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long i = i0 + u;
    if (i < total) {
      const double dl = delta[i];
      // j == 0: eta starts the solve at 0 — write instead of
      // accumulate, so the eta buffer needs no per-solve zeroing pass
      const double et = (j == 0) ? 0.0 : eta[i];
      // snapshots are write-once, re-read only on a (rare) rejection
      // replay: nontemporal stores skip L2 write-allocate, halving
      // the kernel's cache pressure (dominant at 1M-pose scale)
      __builtin_nontemporal_store(et, &eta_snap[(size_t)j * total + i]);
      __builtin_nontemporal_store(dl, &delta_snap[(size_t)j * total + i]);
      eta[i] = fma(coef, dl, et);
      // z is dead until the next dense apply writes it: clear it here
      // instead of in a launch of its own (nullptr on the Jacobi path)
      if (zero_out) zero_out[i] = 0.0;
      if (!stop_pending) {
        const double rn = fma(coef, Hd[i], rvec[i]);
        rvec[i] = rn;
        rr = fma(rn, rn, rr);
      }
    }
  }
  finish_reduction<CF>(ctrl, nblk, stop_pending ? -1 : C_DOT1, rr);
}

template <int CF = CF_NONE>
__global__ void k_tcg_update(double* __restrict__ eta,
                             double* __restrict__ rvec,
                             const double* __restrict__ delta0,
                             const double* __restrict__ Hd,
                             double* __restrict__ eta_snap,
                             double* __restrict__ delta_snap,
                             double* __restrict__ ctrl,
                             long total,
                             double* __restrict__ zero_out,
                             const double* __restrict__ delta1) {
  tcg_update_body<CF>(eta, rvec, delta0, Hd, eta_snap, delta_snap, ctrl,
                      total, zero_out, delta1, (int)gridDim.x);
}

// delta = -z + beta * delta
__global__ void k_tcg_delta(double* __restrict__ delta,
                            const double* __restrict__ z,
                            double* __restrict__ ctrl, long total) {
  if (guarded_off(ctrl, ST_RUN)) return;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  delta[i] = fma(ctrl[C_BETA], delta[i], -z[i]);
}

// step = eta_snap[jstar] + tau*delta_snap[jstar], or current eta
__global__ void k_form_step(double* __restrict__ step,
                            const double* __restrict__ eta,
                            const double* __restrict__ eta_snap,
                            const double* __restrict__ delta_snap,
                            const double* __restrict__ ctrl, long total) {
  if (guarded_off(ctrl, ST_TCG_STOP)) return;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  if (ctrl[C_USE_CURRENT] != 0.0) {
    step[i] = eta[i];
  } else {
    const int j = (int)ctrl[C_JSTAR];
    const double tau = ctrl[C_TAUSTAR];
    step[i] = fma(tau, delta_snap[(size_t)j * total + i],
                  eta_snap[(size_t)j * total + i]);
  }
}

// One trust-region candidate in one launch: k_ctrl_candidate, k_form_step
// and k_polar_affine(X, step, 1, 1) back to back, one thread per pose.
// Thread 0 of every block replays the (at most MAX_TCG entries of)
// Krylov history for itself and hands the selection to its block through
// LDS; the replay reads only slots that this kernel does not write, and
// block 0 alone stores the selection, so no block can see another's
// store. Each thread forms its pose's step tile in registers (the same
// single fma per element as k_form_step), stores it, and retracts
// X + step into Xprop.
template <int D, int R>
__device__ __forceinline__ void candidate_body(
    double* __restrict__ ctrl, double* __restrict__ step,
    const double* __restrict__ eta, const double* __restrict__ eta_snap,
    const double* __restrict__ delta_snap, const double* __restrict__ X,
    double* __restrict__ Xprop, int n) {
  if (guarded_off(ctrl, ST_TCG_STOP)) return;
  __shared__ CandSel sel_sh;
  if (threadIdx.x == 0) {
    sel_sh = ctrl_candidate_replay(ctrl);
    if (blockIdx.x == 0) ctrl_candidate_store(ctrl, sel_sh);
  }
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int dh = D + 1;
  const int jstar = sel_sh.jstar;
  const double tau = sel_sh.taustar;
  const size_t total = (size_t)n * dh * R;
  const size_t base = (size_t)i * dh * R;
  const double* Ei = (jstar < 0 ? eta : eta_snap + (size_t)jstar * total)
                     + base;
  const double* Di = delta_snap + (size_t)(jstar < 0 ? 0 : jstar) * total
                     + base;
  double Mt[dh][R];
  #pragma unroll
  for (int c = 0; c < dh; ++c)
    #pragma unroll
    for (int k = 0; k < R; ++k) {
      double st = Ei[c * R + k];
      if (jstar >= 0) st = fma(tau, Di[c * R + k], st);
      step[base + c * R + k] = st;
      // k_polar_affine's 1 * X, then fma(1, step, .)
      Mt[c][k] = fma(1.0, st, X[base + c * R + k]);
    }
  polar_tile<D, R>(Mt, Xprop + base);
}

template <int D, int R>
__global__ void k_candidate(double* __restrict__ ctrl,
                            double* __restrict__ step,
                            const double* __restrict__ eta,
                            const double* __restrict__ eta_snap,
                            const double* __restrict__ delta_snap,
                            const double* __restrict__ X,
                            double* __restrict__ Xprop, int n) {
  candidate_body<D, R>(ctrl, step, eta, eta_snap, delta_snap, X, Xprop, n);
}

// out = a*A + b*B elementwise (unguarded helper)
__global__ void k_axpby(const double* __restrict__ A,
                        const double* __restrict__ B,
                        double a, double b,
                        double* __restrict__ out, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  double v = a * A[i];
  if (B) v = fma(b, B[i], v);
  out[i] = v;
}

// dots: ctrl[slot] += <A, B>, optionally ctrl[slot2] += <A, C>
__global__ void k_dots(const double* __restrict__ A,
                       const double* __restrict__ B,
                       const double* __restrict__ C,
                       double* __restrict__ ctrl,
                       int slot, int slot2, long total, int guard) {
  if (guarded_off(ctrl, guard)) return;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  double d0 = 0.0, d1 = 0.0;
  if (i < total) {
    const double a = A[i];
    d0 = a * B[i];
    if (C) d1 = a * C[i];
  }
  block_reduce_atomic(d0, ctrl + slot);
  if (C && slot2 >= 0) block_reduce_atomic(d1, ctrl + slot2);
}

// ---------------------------------------------------------------------
// Single-wave tCG control kernels (device-side branch logic)
// ---------------------------------------------------------------------
__global__ void k_ctrl_init(double* ctrl, double tol, double Delta0,
                            double theta, double kappa) {
  if (threadIdx.x == 0) ctrl_body_init(ctrl, tol, Delta0, theta, kappa);
}

// Standalone launch of one control tail (ctrl_tail_z0/alpha/rr/beta):
// what DPO_NO_CF=1 runs after the producing reduction kernel instead of
// the tail fused into that kernel's last block.
template <int CF>
__global__ void k_ctrl_tail(double* ctrl) {
  if (threadIdx.x == 0) run_ctrl_tail(CF, ctrl, TailArgs());
}

template <int CF>
static void launch_ctrl_tail(double* ctrl, hipStream_t s) {
  hipLaunchKernelGGL((k_ctrl_tail<CF>), dim3(1), dim3(64), 0, s, ctrl);
}

// end of the unrolled loop: cap at max_inner
__device__ __forceinline__ void ctrl_tcg_end_body(double* ctrl) {
  if (threadIdx.x != 0) return;
  if (ctrl[C_STATUS] != (double)ST_RUN) return;
  ctrl[C_STATUS] = (double)ST_TCG_STOP;
  ctrl[C_J] = ctrl[C_ITER];
  ctrl[C_HLEN] = ctrl[C_ITER];
  ctrl[C_USE_CURRENT] = 1.0;
}
__global__ void k_ctrl_tcg_end(double* ctrl) { ctrl_tcg_end_body(ctrl); }

// candidate selection for the current radius: replay the stored Krylov
// scalars, find the truncation point and the model decrease.
__global__ void k_ctrl_candidate(double* ctrl) {
  if (threadIdx.x != 0) return;
  if (ctrl[C_STATUS] != (double)ST_TCG_STOP) return;
  ctrl_candidate_store(ctrl, ctrl_candidate_replay(ctrl));
}

// acceptance test after f(X_prop) dots (C_DOT0 = <QXp, Xp>, C_DOT2 = <G, Xp>)
__global__ void k_ctrl_accept(double* ctrl, double accept_rho) {
  if (threadIdx.x == 0) ctrl_body_accept(ctrl, accept_rho);
}

// shrink the radius after a rejection (host re-enqueues the candidate set)
__global__ void k_ctrl_shrink(double* ctrl) {
  if (threadIdx.x != 0) return;
  if (ctrl[C_STATUS] != (double)ST_TCG_STOP) return;
  ctrl[C_RADIUS] *= 0.25;
  ctrl[C_SHRINKS] += 1.0;
}

// ---------------------------------------------------------------------
// Assembly kernels
// ---------------------------------------------------------------------
// Q values: vals[slot] += w[edge_of[c]] * blocks[c]  (scatter-add)
__global__ void k_q_assemble(double* __restrict__ vals,
                             const double* __restrict__ blocks,
                             const long* __restrict__ slots,
                             const long* __restrict__ edge_of,
                             const double* __restrict__ w,
                             int ncontrib, int bsz) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)ncontrib * bsz) return;
  const int c = i / bsz, e = i % bsz;
  atomicAdd(&vals[slots[c] * bsz + e], w[edge_of[c]] * blocks[i]);
}

// G values: Gt[local_pose[e]] += -w[e] * E0[e] @ nbr[slot[e]]
// one thread per (edge, c, k) output element
__device__ __forceinline__ void g_assemble_body(
    double* __restrict__ Gt, const double* __restrict__ E0,
    const long* __restrict__ local_pose, const long* __restrict__ nbr_slot,
    const double* __restrict__ nbr, const double* __restrict__ w, int ne,
    int dh, int r) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)ne * dh * r) return;
  const int e = i / (dh * r);
  const int t = i % (dh * r);
  const int c = t / r, k = t % r;
  const double* Ee = E0 + (size_t)e * dh * dh;
  const double* Xn = nbr + (size_t)nbr_slot[e] * dh * r;
  double acc = 0.0;
  for (int b = 0; b < dh; ++b) acc = fma(Ee[c * dh + b], Xn[b * r + k], acc);
  atomicAdd(&Gt[((size_t)local_pose[e] * dh + c) * r + k], -w[e] * acc);
}

__global__ void k_g_assemble(double* __restrict__ Gt,
                             const double* __restrict__ E0,
                             const long* __restrict__ local_pose,
                             const long* __restrict__ nbr_slot,
                             const double* __restrict__ nbr,
                             const double* __restrict__ w,
                             int ne, int dh, int r) {
  g_assemble_body(Gt, E0, local_pose, nbr_slot, nbr, w, ne, dh, r);
}

// ---------------------------------------------------------------------
// GNC-TLS loop-closure re-weighting (reference PGOAgent::
// updateLoopClosuresWeights, PGOAgent.cpp:1181-1245, weight formula
// DPGO_robust.cpp:49-62). One thread per edge; endpoints are rows of X
// (local poses) or of the packed neighbor buffer (shared edges).
// Residual on the LIFTED variables: r^2 = kappa ||R^T Y1t - Y2t||_F^2
//                                      + tau ||p2 - p1 - t^T Y1t||^2.
// update_mask == 0 keeps the current weight (known inliers, non-owned
// shared edges under the owner-computes rule).
// ---------------------------------------------------------------------
template <int D, int R>
__global__ void k_gnc_weights(const double* __restrict__ X,
                              const double* __restrict__ nbr,
                              const long* __restrict__ e1_idx,
                              const unsigned char* __restrict__ e1_nbr,
                              const long* __restrict__ e2_idx,
                              const unsigned char* __restrict__ e2_nbr,
                              const double* __restrict__ Rm,
                              const double* __restrict__ tm,
                              const double* __restrict__ kappa,
                              const double* __restrict__ tau,
                              const unsigned char* __restrict__ update_mask,
                              const long* __restrict__ widx,
                              double* __restrict__ weights,
                              int ne, double mu, double barc_sq) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ne) return;
  if (!update_mask[e]) return;
  constexpr int dh = D + 1;
  const double* P1 = (e1_nbr[e] ? nbr : X) + (size_t)e1_idx[e] * dh * R;
  const double* P2 = (e2_nbr[e] ? nbr : X) + (size_t)e2_idx[e] * dh * R;
  const double* Re = Rm + (size_t)e * D * D;
  const double* te = tm + (size_t)e * D;
  double rot_err = 0.0, tran_err = 0.0;
  #pragma unroll
  for (int k = 0; k < R; ++k) {
    #pragma unroll
    for (int b = 0; b < D; ++b) {
      // (Y1 R)^T row b = sum_a R[a][b] * Y1t[a][:]
      double v = 0.0;
      #pragma unroll
      for (int a = 0; a < D; ++a) v = fma(Re[a * D + b], P1[a * R + k], v);
      const double diff = v - P2[b * R + k];
      rot_err = fma(diff, diff, rot_err);
    }
    double tv = P2[D * R + k] - P1[D * R + k];
    #pragma unroll
    for (int a = 0; a < D; ++a) tv = fma(-te[a], P1[a * R + k], tv);
    tran_err = fma(tv, tv, tran_err);
  }
  const double r_sq = kappa[e] * rot_err + tau[e] * tran_err;
  // GNC-TLS weight (eq. 14)
  const double upper = (mu + 1.0) / mu * barc_sq;
  const double lower = mu / (mu + 1.0) * barc_sq;
  double w;
  if (r_sq >= upper) w = 0.0;
  else if (r_sq <= lower) w = 1.0;
  else w = sqrt(barc_sq * mu * (mu + 1.0) / r_sq) - mu;
  weights[widx[e]] = w;
}

// ---------------------------------------------------------------------
// (d, r) dispatch: the supported compile-time shapes. SE(2): d=2,
// r in 2..6; SE(3): d=3, r in 3..8. Everything the reference exercises
// (r=5 RBCD, r=d batch) is covered; exotic shapes abort loudly.
// ---------------------------------------------------------------------
#define DPO_FOREACH_DR(F) \
  F(2, 2) F(2, 3) F(2, 4) F(2, 5) F(2, 6) \
  F(3, 3) F(3, 4) F(3, 5) F(3, 6) F(3, 7) F(3, 8)

// Calls f(integral_constant<int, D>, integral_constant<int, R>) for the
// supported pair equal to (d, r); false (f not called) for any other.
// f is a generic lambda; its arguments convert to constant expressions
// (constexpr int D = Dc), so it can name k_foo<D, R>.
template <class F>
static bool dispatch_dr(int d, int r, F&& f) {
#define DPO_DISPATCH_ONE(D, R)                            \
  if (d == D && r == R) {                                 \
    f(std::integral_constant<int, D>{},                   \
      std::integral_constant<int, R>{});                  \
    return true;                                          \
  }
  DPO_FOREACH_DR(DPO_DISPATCH_ONE)
#undef DPO_DISPATCH_ONE
  return false;
}

// r alone, for kernels that do not depend on d: every r of the list.
template <class F>
static bool dispatch_r(int r, F&& f) {
  auto g = [&](auto, auto Rc) { f(Rc); };
  return dispatch_dr(2, r, g) || dispatch_dr(3, r, g);
}

static inline int blocks_for(long total, int bs) {
  return (int)((total + bs - 1) / bs);
}

static void dpo_bad_shape(int d, int r) {
  fprintf(stderr, "dpo_ops: unsupported (d=%d, r=%d) kernel shape\n", d, r);
  abort();
}

static void launch_spmm(const int* rp, const int* ci, const double* vals,
                        int n, int d, int r, const double* X, double* out,
                        const double* ctrl, int guard, hipStream_t s) {
  const int dh = d + 1;
  const int tile = dh * r;
  const int grid = blocks_for(n, 256 / tile);
  if (!dispatch_dr(d, r, [&](auto Dc, auto Rc) {
        hipLaunchKernelGGL((k_bsr_spmm<Dc + 1, Rc>), dim3(grid), dim3(256),
                           0, s, rp, ci, vals, X, out, n, ctrl, guard);
      }))
    hipLaunchKernelGGL(k_bsr_spmm_gen, dim3(grid), dim3(256), 0, s,
                       rp, ci, vals, X, out, n, dh, r, ctrl, guard);
}

// Wide-variant selection: element-per-thread (dh*r threads per pose)
// for large agents, where the thread-per-pose kernel's n/64 waves are
// too few to hide HBM latency (1M-pose profile, round 1); the fused
// thread-per-pose kernel stays the default for the (launch-latency-
// bound) small-agent regime. DPO_HESS_WIDE=0/1 forces either path.
static inline bool hess_use_wide(int n) {
  static const int mode = []() {
    const char* v = getenv("DPO_HESS_WIDE");
    return v ? atoi(v) : -1;
  }();
  if (mode == 0) return false;
  if (mode == 1) return true;
  // Measured (profiles/r2c_*): the thread-per-pose kernel runs at
  // ~HBM roofline even at 125k poses/agent (concurrent agents supply
  // the missing waves), while the element-per-thread layout pays ~5x
  // redundant Q-row reads. Wide stays opt-in for experiments.
  return false;
}

template <int CF = CF_NONE>
static void launch_proj_dots(const double* X, const double* V,
                             const double* G, double* out,
                             const double* dotWith, double* ctrl,
                             int n, int d, int r, int dot_slot,
                             int dot_slot2, int guard, hipStream_t s) {
  const bool wide = hess_use_wide(n);
  if (!dispatch_dr(d, r, [&](auto Dc, auto Rc) {
        constexpr int D = Dc, R = Rc;
        if (wide) {
          constexpr int PB = 256 / ((D + 1) * R);
          hipLaunchKernelGGL((k_proj_wide<D, R, CF>),
                             dim3(blocks_for(n, PB)), dim3(256), 0, s,
                             X, V, G, out, dotWith, ctrl, n, dot_slot,
                             dot_slot2, guard);
        } else {
          hipLaunchKernelGGL((k_proj_dots<D, R, CF>),
                             dim3(blocks_for(n, 256)), dim3(256), 0, s,
                             X, V, G, out, dotWith, ctrl, n, dot_slot,
                             dot_slot2, guard);
        }
      }))
    dpo_bad_shape(d, r);
}

static void launch_polar(const double* A, const double* B, const double* C,
                         double ca, double cb, double cc, double* out,
                         int n, int d, int r, const double* ctrl, int guard,
                         hipStream_t s) {
  if (!dispatch_dr(d, r, [&](auto Dc, auto Rc) {
        hipLaunchKernelGGL((k_polar_affine<Dc, Rc>),
                           dim3(blocks_for(n, 256)), dim3(256), 0, s,
                           A, B, C, ca, cb, cc, out, n, ctrl, guard);
      }))
    dpo_bad_shape(d, r);
}

template <int MODE, int CF = CF_NONE, int AUX = 0>
static void launch_hess_fused(const int* rp, const int* ci,
                              const double* vals, const double* V,
                              const double* X, const double* G,
                              double* out, const double* dotW,
                              double* ctrl, int n, int d, int r,
                              int dot_slot, int dot_slot2, int guard,
                              hipStream_t s, int dot_slot3 = -1,
                              double* out2 = nullptr,
                              double* zero_out = nullptr,
                              const TailArgs& ta = TailArgs()) {
  // AUX == 2 (folded direction) exists for the thread-per-pose kernel
  // only; its callers do not fold when the wide kernels are selected
  const bool wide = AUX != 2 && hess_use_wide(n);
  if (!dispatch_dr(d, r, [&](auto Dc, auto Rc) {
        constexpr int D = Dc, R = Rc;
        if (wide) {
          constexpr int PB = 256 / ((D + 1) * R);
          hipLaunchKernelGGL((k_hess_wide<D, R, MODE, CF, AUX == 2 ? 0 : AUX>),
                             dim3(blocks_for(n, PB)), dim3(256), 0, s,
                             rp, ci, vals, V, X, G, out, dotW, ctrl, n,
                             dot_slot, dot_slot2, dot_slot3, guard, out2,
                             zero_out, ta);
        } else {
          hipLaunchKernelGGL((k_hess_fused<D, R, MODE, CF, AUX>),
                             dim3(blocks_for(n, 256)), dim3(256), 0, s,
                             rp, ci, vals, V, X, G, out, dotW, ctrl, n,
                             dot_slot, dot_slot2, dot_slot3, guard, out2,
                             zero_out, ta);
        }
      }))
    dpo_bad_shape(d, r);
}

// Graph-safe zero / device->pinned-host copy. hipMemsetAsync and
// hipMemcpyAsync become SDMA-engine nodes inside a captured hipGraph;
// compute<->SDMA dependencies in replayed graphs are part of the same
// ROCm 7.2 ordering fragility the launch fences work around, so the
// captured bodies use plain kernels only.
__device__ __forceinline__ void dzero_body(double* p, long n) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0.0;
}
__global__ void k_dzero(double* p, long n) { dzero_body(p, n); }
// two buffers in one launch (the solve head's G_buf and control block)
__device__ __forceinline__ void dzero2_body(double* p, long n, double* q,
                                            long m) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0.0;
  if (i < m) q[i] = 0.0;
}
__global__ void k_dzero2(double* p, long n, double* q, long m) {
  dzero2_body(p, n, q, m);
}
__global__ void k_ctrl_to_host(const double* __restrict__ src,
                               double* __restrict__ dst, int n) {
  // one wave copies all n slots (n = CTRL_SIZE exceeds the wave)
  for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}

static inline void dzero(double* p, long n, hipStream_t s) {
  hipLaunchKernelGGL(k_dzero, dim3(blocks_for(n, 256)), dim3(256), 0, s, p,
                     n);
}

// Overwrites every element of Z unless guarded off (then Z is untouched).
static void launch_precond_dense(const float* Minv, const double* V,
                                 double* Z, int N, int r,
                                 const double* ctrl, int guard,
                                 hipStream_t s) {
  const int strips = precond_dense_strips(N);
  const bool vec = precond_dense_vec_ok(Minv, N);
  if (!dispatch_r(r, [&](auto Rc) {
        if (vec)
          hipLaunchKernelGGL((k_precond_dense<Rc, true>), dim3(strips),
                             dim3(256), 0, s, Minv, V, Z, N, ctrl, guard);
        else
          hipLaunchKernelGGL((k_precond_dense<Rc, false>), dim3(strips),
                             dim3(256), 0, s, Minv, V, Z, N, ctrl, guard);
      }))
    dpo_bad_shape(-1, r);
}

static void launch_precond_jacobi(const double* L, const double* V,
                                  double* Z, int n, int dh, int r,
                                  const double* ctrl, int guard,
                                  hipStream_t s) {
  const int grid = blocks_for((long)n * r, 256);
  if (dh == 3)
    hipLaunchKernelGGL((k_precond_jacobi<3>), dim3(grid), dim3(256), 0, s,
                       L, V, Z, n, r, ctrl, guard);
  else if (dh == 4)
    hipLaunchKernelGGL((k_precond_jacobi<4>), dim3(grid), dim3(256), 0, s,
                       L, V, Z, n, r, ctrl, guard);
  else
    dpo_bad_shape(dh - 1, r);
}

template <int CF>
static void launch_tcg_update(double* eta, double* rvec, const double* delta,
                              const double* Hd, double* eta_snap,
                              double* delta_snap, double* ctrl, long total,
                              double* zero_out, hipStream_t s,
                              const double* delta1 = nullptr) {
  hipLaunchKernelGGL((k_tcg_update<CF>),
                     dim3(blocks_for((total + 3) / 4, 256)), dim3(256), 0, s,
                     eta, rvec, delta, Hd, eta_snap, delta_snap, ctrl, total,
                     zero_out, delta1);
}

extern "C" {

void dpo_bsr_spmm(const int* row_ptr, const int* col_idx, const double* vals,
                  int n, int dh, const double* X, double* out, int r,
                  const double* ctrl, int guard, void* stream) {
  launch_spmm(row_ptr, col_idx, vals, n, dh - 1, r, X, out, ctrl, guard,
              (hipStream_t)stream);
}

void dpo_bsr_spmm_mfma(const int* grp_ptr, const int* grp_cols,
                       const int* grp_blk, const double* vals,
                       const double* X, double* out, int ngroups, int n,
                       int r, void* stream) {
  const int waves_per_block = 4;
  const int grid = (ngroups + waves_per_block - 1) / waves_per_block;
  hipLaunchKernelGGL(k_bsr_spmm_mfma_d3, dim3(grid),
                     dim3(64 * waves_per_block), 0, (hipStream_t)stream,
                     grp_ptr, grp_cols, grp_blk, vals, X, out, ngroups,
                     n, r);
}

void dpo_proj_dots(const double* X, const double* V, const double* G,
                   double* out, const double* dotWith, double* ctrl,
                   int n, int d, int r, int dot_slot, int dot_slot2,
                   int neg, int guard, void* stream) {
  (void)neg;  // the negated variant is realized by k_tcg_delta instead
  launch_proj_dots(X, V, G, out, dotWith, ctrl, n, d, r, dot_slot,
                   dot_slot2, guard, (hipStream_t)stream);
}

void dpo_polar_affine(const double* A, const double* B, const double* C,
                      double ca, double cb, double cc, double* out,
                      int n, int d, int r, const double* ctrl, int guard,
                      void* stream) {
  launch_polar(A, B, C, ca, cb, cc, out, n, d, r, ctrl, guard,
               (hipStream_t)stream);
}

void dpo_precond_dense(const float* Minv, const double* V, double* Z,
                       int N, int r, const double* ctrl, int guard,
                       void* stream) {
  // stand-alone entry: Z is exactly zero when the launch is guarded off.
  // Kernel (not hipMemsetAsync): callers may capture this into graphs,
  // which must stay free of SDMA nodes (see fence comment)
  dzero(Z, (long)N * r, (hipStream_t)stream);
  launch_precond_dense(Minv, V, Z, N, r, ctrl, guard, (hipStream_t)stream);
}

void dpo_precond_jacobi(const double* L, const double* V, double* Z,
                        int n, int dh, int r, const double* ctrl, int guard,
                        void* stream) {
  launch_precond_jacobi(L, V, Z, n, dh, r, ctrl, guard,
                        (hipStream_t)stream);
}

void dpo_tcg_update(double* eta, double* rvec, const double* delta,
                    const double* Hd, double* eta_snap, double* delta_snap,
                    double* ctrl, long total, void* stream) {
  launch_tcg_update<CF_NONE>(eta, rvec, delta, Hd, eta_snap, delta_snap,
                             ctrl, total, nullptr, (hipStream_t)stream);
}

void dpo_tcg_delta(double* delta, const double* z, double* ctrl, long total,
                   void* stream) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_tcg_delta, dim3(blocks_for(total, 256)), dim3(256),
                     0, s, delta, z, ctrl, total);
}

void dpo_form_step(double* step, const double* eta, const double* eta_snap,
                   const double* delta_snap, const double* ctrl, long total,
                   void* stream) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_form_step, dim3(blocks_for(total, 256)), dim3(256),
                     0, s, step, eta, eta_snap, delta_snap, ctrl, total);
}

void dpo_axpby(const double* A, const double* B, double a, double b,
               double* out, long total, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_axpby, dim3(blocks_for(total, 256)), dim3(256),
                     0, s, A, B, a, b, out, total);
}

void dpo_dots(const double* A, const double* B, const double* C,
              double* ctrl, int slot, int slot2, long total, int guard,
              void* stream) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_dots, dim3(blocks_for(total, 256)), dim3(256), 0, s,
                     A, B, C, ctrl, slot, slot2, total, guard);
}

void dpo_ctrl_init(double* ctrl, double tol, double Delta0, double theta,
                   double kappa, void* stream) {
  hipLaunchKernelGGL(k_ctrl_init, dim3(1), dim3(64), 0,
                     (hipStream_t)stream, ctrl, tol, Delta0, theta, kappa);
}
void dpo_ctrl_z0(double* ctrl, void* stream) {
  launch_ctrl_tail<CF_Z0>(ctrl, (hipStream_t)stream);
}
void dpo_ctrl_alpha(double* ctrl, void* stream) {
  launch_ctrl_tail<CF_ALPHA>(ctrl, (hipStream_t)stream);
}
void dpo_ctrl_rr(double* ctrl, void* stream) {
  launch_ctrl_tail<CF_RR>(ctrl, (hipStream_t)stream);
}
void dpo_ctrl_beta(double* ctrl, void* stream) {
  launch_ctrl_tail<CF_BETA>(ctrl, (hipStream_t)stream);
}
void dpo_ctrl_tcg_end(double* ctrl, void* stream) {
  hipLaunchKernelGGL(k_ctrl_tcg_end, dim3(1), dim3(64), 0,
                     (hipStream_t)stream, ctrl);
}
void dpo_ctrl_candidate(double* ctrl, void* stream) {
  hipLaunchKernelGGL(k_ctrl_candidate, dim3(1), dim3(64), 0,
                     (hipStream_t)stream, ctrl);
}
void dpo_ctrl_accept(double* ctrl, double accept_rho, void* stream) {
  hipLaunchKernelGGL(k_ctrl_accept, dim3(1), dim3(64), 0,
                     (hipStream_t)stream, ctrl, accept_rho);
}
void dpo_ctrl_shrink(double* ctrl, void* stream) {
  hipLaunchKernelGGL(k_ctrl_shrink, dim3(1), dim3(64), 0,
                     (hipStream_t)stream, ctrl);
}

void dpo_q_assemble(double* vals, const double* blocks, const long* slots,
                    const long* edge_of, const double* w, int ncontrib,
                    int bsz, long nnzb, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  DPO_CHECK(hipMemsetAsync(vals, 0, (size_t)nnzb * bsz * sizeof(double), s));
  hipLaunchKernelGGL(k_q_assemble,
                     dim3(blocks_for((long)ncontrib * bsz, 256)), dim3(256),
                     0, s, vals, blocks, slots, edge_of, w, ncontrib, bsz);
}

void dpo_g_assemble(double* Gt, const double* E0, const long* local_pose,
                    const long* nbr_slot, const double* nbr, const double* w,
                    int ne, int dh, int r, long N, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  DPO_CHECK(hipMemsetAsync(Gt, 0, (size_t)N * r * sizeof(double), s));
  hipLaunchKernelGGL(k_g_assemble,
                     dim3(blocks_for((long)ne * dh * r, 256)), dim3(256),
                     0, s, Gt, E0, local_pose, nbr_slot, nbr, w, ne, dh, r);
}

int dpo_ctrl_size() { return CTRL_SIZE; }

void dpo_gnc_weights(const double* X, const double* nbr, const long* e1_idx,
                     const unsigned char* e1_nbr, const long* e2_idx,
                     const unsigned char* e2_nbr, const double* Rm,
                     const double* tm, const double* kappa,
                     const double* tau, const unsigned char* update_mask,
                     const long* widx, double* weights, int ne, int d,
                     int r, double mu, double barc_sq, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!dispatch_dr(d, r, [&](auto Dc, auto Rc) {
        hipLaunchKernelGGL((k_gnc_weights<Dc, Rc>),
                           dim3(blocks_for(ne, 256)), dim3(256), 0, s,
                           X, nbr, e1_idx, e1_nbr, e2_idx, e2_nbr, Rm, tm,
                           kappa, tau, update_mask, widx, weights, ne, mu,
                           barc_sq);
      }))
    dpo_bad_shape(d, r);
}

}  // extern "C"

// =====================================================================
// C++ solver orchestration: the full RBCD trust-region local solve and
// the per-round evaluation, enqueued from native code (one Python call
// per solve instead of ~100). This is the MI355X-native runtime
// replacement for the reference's ROPTLIB-driven QuadraticOptimizer
// (QuadraticOptimizer.cpp:61-122).
// =====================================================================

// combine kernel: out[0..2] = [f, 0.5<X,G>, gn2] from dot slots
__global__ void k_eval_combine(double* __restrict__ ctrl,
                               double* __restrict__ out) {
  if (threadIdx.x == 0) ctrl_body_eval(ctrl, out);
}

// One cached hipGraph exec for a fixed-pointer enqueue sequence.
struct GraphCache {
  hipGraphExec_t exec = nullptr;
  const void* key[4] = {};
  int replays = 0;
  // Periodic graph-exec refresh. The "degradation after a few hundred
  // replays" this originally worked around is now attributed to the
  // SDMA-node / launch-ordering bugs fixed by the fences and
  // kernels-only bodies; the refresh is kept as cheap insurance
  // (amortized ~1%) and is tunable via DPO_MAX_REPLAYS.
  static int max_replays() {
    static const int v = [] {
      const char* e = getenv("DPO_MAX_REPLAYS");
      return e ? atoi(e) : 128;
    }();
    return v;
  }
  void reset() {
    if (exec) {
      dpo_ignore(hipGraphExecDestroy(exec));
      exec = nullptr;
    }
  }
};

// Replay the cached graph on stream s. On a key change (or past the
// refresh limit) first re-record it: body(cap) enqueues the sequence on
// the capture stream. Returns false — nothing enqueued on s — when
// capture/instantiation is unavailable; the caller then runs eagerly.
template <class Body>
static bool graph_cache_launch(GraphCache& g, const void* const (&key)[4],
                               hipStream_t cap, hipStream_t s, Body body) {
  const bool match = g.exec && memcmp(key, g.key, sizeof(key)) == 0
                     && g.replays < GraphCache::max_replays();
  if (!match) {
    g.reset();
    g.replays = 0;
    hipGraph_t graph = nullptr;
    hipError_t rc = hipStreamBeginCapture(
        cap, hipStreamCaptureModeThreadLocal);
    if (rc == hipSuccess) {
      body(cap);
      rc = hipStreamEndCapture(cap, &graph);
    }
    // a failed capture can leave the stream capturing: close it out
    hipStreamCaptureStatus capst = hipStreamCaptureStatusNone;
    dpo_ignore(hipStreamIsCapturing(cap, &capst));
    if (capst != hipStreamCaptureStatusNone) {
      hipGraph_t dead = nullptr;
      dpo_ignore(hipStreamEndCapture(cap, &dead));
      if (dead) dpo_ignore(hipGraphDestroy(dead));
    }
    if (rc == hipSuccess && graph) {
      rc = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
      dpo_ignore(hipGraphDestroy(graph));
    }
    dpo_ignore(hipGetLastError());  // clear sticky capture-related error state
    if (rc != hipSuccess || !g.exec) {
      g.exec = nullptr;
      return false;
    }
    memcpy(g.key, key, sizeof(key));
  }
  g.replays++;
  DPO_CHECK(hipGraphLaunch(g.exec, s));
  return true;
}

struct DpoCtx {
  int n, d, r, dh, N, max_inner;
  long total;
  double *W, *grad, *eta, *delta, *delta1, *rvec, *z, *Hd, *step, *Xprop;
  double *eta_snap, *delta_snap, *ctrl;
  double *ctrl_host;      // pinned
  double *ctrl_host_dev;  // device-side view of ctrl_host (mapped)
  // borrowed problem pointers (owned by torch tensors on the Python side)
  const int *q_rp = nullptr, *q_ci = nullptr;
  const double *q_vals = nullptr;
  const double *Gt = nullptr;
  const float *Minv = nullptr;
  const double *Ljac = nullptr;
  // G-assembly structure (owned by torch tensors)
  const double *g_E0 = nullptr;
  const long *g_local_pose = nullptr, *g_nbr_slot = nullptr;
  const double *g_w = nullptr;
  int g_ne = 0;
  double *G_buf = nullptr;  // ctx-owned (N, r) linear-term buffer
  // hipGraph caches for the fixed-pointer round sequences. Keyed by the
  // operand pointers; invalidated whenever set_problem/set_gdata change
  // them (preconditioner refresh, Q rebuild keep the same buffers).
  GraphCache solve_graph, eval_graph;
  // second segment of a segmented solve (see solve_segment()): the tCG
  // iterations past the primary graph's + the tail. Same key and
  // refresh rule as solve_graph; captured on first need.
  GraphCache cont_graph;
  // host-side statistics, updated where ctrl_host is read anyway
  long n_solves = 0, n_conts = 0;
  long hlen_hist[MAX_TCG + 1] = {};
  // private stream used only for RECORDING captures (the legacy default
  // stream cannot be captured); graphs replay on the caller's stream.
  hipStream_t cap_stream = nullptr;
  // per-agent execution stream + events: lets concurrent agents' solves
  // and the per-round evaluations overlap on the GPU (colored schedule,
  // 8-agent eval fan-out) while staying ordered against the caller's
  // (torch) stream via events.
  hipStream_t exec_stream = nullptr;
  hipEvent_t start_event = nullptr;
  hipEvent_t done_event = nullptr;
  // state of an in-flight async solve
  double pend_tol = 0, pend_Delta0 = 0, pend_rho = 0;
  double* pend_X = nullptr;
  const double* pend_nbr = nullptr;
  // data-flow fence slots (see k_fence_* above)
  unsigned int* fences = nullptr;
  // fixed 3-double eval destination for the group fan-out path (a
  // stable pointer keeps the eval graph cache hot)
  double* eval3 = nullptr;
  // Advanced whenever a pointer that a batch descriptor copies out of this
  // context changes (problem / G-structure setters); a DpoGroup compares
  // it before each batched launch and rebuilds its descriptors and graphs
  // when it moved. Re-binding the same buffers (a Q rebuild or a GNC
  // re-weighting in place) leaves it alone. The linear term does not
  // count: set_problem resets Gt and the round assembly sets it again,
  // which invalidates the per-agent graphs (they hold Gt as an argument)
  // but not a descriptor, which always names G_buf.
  long desc_stamp = 0;
  void invalidate_graphs() {
    solve_graph.reset();
    cont_graph.reset();
    eval_graph.reset();
  }
};

// --- data-flow fences around hipGraph launches ----------------------
// ROCm 7.2 on gfx950: a hipGraphLaunch intermittently fails to order
// against work enqueued on other streams via hipStreamWaitEvent (and,
// on the legacy stream, against prior eager work), executing the graph
// early/concurrently. Observed as rare stale/garbage reads in the
// round pipeline (bisected: eager-everything is stable, every failing
// configuration launches a graph whose cross-stream ordering is
// load-bearing). Instead of depending on launch ordering at all, each
// graph carries explicit data-flow fences:
//   producer stream:  k_fence_signal(IN)   (eager kernel — reliable)
//   graph first node: k_fence_wait(IN)     (spins until signalled)
//   graph last node:  k_fence_signal(OUT)
//   consumer stream:  k_fence_wait(OUT)    (eager kernel after launch)
// so even a misordered launch blocks on its first node until its
// inputs are ready, and downstream eager work blocks until the graph
// really finished. Cost: ~2 one-wave kernels per launch (<2 us).
enum { F_SOLVE_IN = 0, F_SOLVE_OUT = 1, F_EVAL_IN = 2, F_EVAL_OUT = 3,
       F_NUM = 4 };

__global__ void k_fence_signal(unsigned int* f) {
  if (threadIdx.x == 0)
    __hip_atomic_store(f, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void k_fence_wait(unsigned int* f) {
  if (threadIdx.x == 0) {
    long spins = 0;
    while (__hip_atomic_load(f, __ATOMIC_ACQUIRE,
                             __HIP_MEMORY_SCOPE_AGENT) == 0u) {
      __builtin_amdgcn_s_sleep(64);
      // ~50 s at ~1.7us/iter: a lost signal is a programming error —
      // fail loudly (aborted kernel surfaces on the next sync) rather
      // than silently proceeding on unordered data.
      if (++spins > 30000000L) __builtin_trap();
    }
    __hip_atomic_store(f, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

static inline void fence_signal(DpoCtx* c, int which, hipStream_t s) {
  hipLaunchKernelGGL(k_fence_signal, dim3(1), dim3(64), 0, s,
                     c->fences + which);
}
static inline void fence_wait(DpoCtx* c, int which, hipStream_t s) {
  hipLaunchKernelGGL(k_fence_wait, dim3(1), dim3(64), 0, s,
                     c->fences + which);
}

// The linear term a round assembly leaves bound: G_buf when the agent has
// shared edges, none otherwise. ctx_assemble_g sets it when it enqueues
// the assembly; the batched path, whose kernels take it from the
// descriptor, sets it through the same function (the per-agent shrink
// loop of solve_postsync reads c->Gt).
static inline const double* ctx_bind_round_g(DpoCtx* c) {
  c->Gt = c->g_ne > 0 ? c->G_buf : nullptr;
  return c->Gt;
}

// with_ctrl: the launch that clears G_buf clears the control block too
// (solve head).
static void ctx_assemble_g(DpoCtx* c, const double* nbr, hipStream_t s,
                           bool with_ctrl = false) {
  if (!ctx_bind_round_g(c)) {
    if (with_ctrl) dzero(c->ctrl, CTRL_SIZE, s);
    return;
  }
  if (with_ctrl) {
    const long m = c->total > CTRL_SIZE ? c->total : CTRL_SIZE;
    hipLaunchKernelGGL(k_dzero2, dim3(blocks_for(m, 256)), dim3(256), 0, s,
                       c->G_buf, c->total, c->ctrl, (long)CTRL_SIZE);
  } else {
    dzero(c->G_buf, c->total, s);
  }
  hipLaunchKernelGGL(k_g_assemble,
                     dim3(((long)c->g_ne * c->dh * c->r + 255) / 256),
                     dim3(256), 0, s, c->G_buf, c->g_E0, c->g_local_pose,
                     c->g_nbr_slot, nbr, c->g_w, c->g_ne, c->dh, c->r);
}

// The buffer the solve body clears in front of each dense apply: z on the
// dense path, nullptr on the Jacobi path. The strip apply overwrites z
// and no longer needs it; the clearing stays until its tests move.
static inline double* ctx_prezero_z(const DpoCtx* c) {
  return c->Minv ? c->z : nullptr;
}

// Solve-body preconditioner apply into c->z.
static void ctx_precond(DpoCtx* c, const double* V, double* Z,
                        hipStream_t s) {
  if (c->Minv)
    launch_precond_dense(c->Minv, V, Z, c->N, c->r, c->ctrl, ST_RUN, s);
  else
    launch_precond_jacobi(c->Ljac, V, Z, c->n, c->dh, c->r, c->ctrl,
                          ST_RUN, s);
}

// k_hess_fused / k_hess_wide on the bound problem's Q.
template <int MODE, int CF = CF_NONE, int AUX = 0>
static void ctx_hess(DpoCtx* c, const double* V, const double* X,
                     const double* G, double* out, const double* dotW,
                     int dot_slot, int dot_slot2, int guard, hipStream_t s,
                     int dot_slot3 = -1, double* out2 = nullptr,
                     double* zero_out = nullptr,
                     const TailArgs& ta = TailArgs()) {
  launch_hess_fused<MODE, CF, AUX>(c->q_rp, c->q_ci, c->q_vals, V, X, G, out,
                                   dotW, c->ctrl, c->n, c->d, c->r, dot_slot,
                                   dot_slot2, guard, s, dot_slot3, out2,
                                   zero_out, ta);
}

extern "C" {

void* dpo_ctx_create(int n, int d, int r, int max_inner) {
  DpoCtx* c = new DpoCtx();
  c->n = n; c->d = d; c->r = r; c->dh = d + 1;
  c->N = c->dh * n; c->max_inner = max_inner;
  c->total = (long)c->N * r;
  size_t vb = (size_t)c->total * sizeof(double);
  DPO_CHECK(hipMalloc(&c->W, vb));
  DPO_CHECK(hipMalloc(&c->grad, vb));
  DPO_CHECK(hipMalloc(&c->eta, vb));
  DPO_CHECK(hipMalloc(&c->delta, vb));
  DPO_CHECK(hipMalloc(&c->delta1, vb));
  DPO_CHECK(hipMalloc(&c->rvec, vb));
  DPO_CHECK(hipMalloc(&c->z, vb));
  DPO_CHECK(hipMalloc(&c->Hd, vb));
  DPO_CHECK(hipMalloc(&c->step, vb));
  DPO_CHECK(hipMalloc(&c->Xprop, vb));
  DPO_CHECK(hipMalloc(&c->eta_snap, vb * (max_inner + 1)));
  DPO_CHECK(hipMalloc(&c->delta_snap, vb * (max_inner + 1)));
  DPO_CHECK(hipMalloc(&c->ctrl, CTRL_SIZE * sizeof(double)));
  // hipMalloc does not clear: an evaluation before the first solve adds
  // its dot products into C_DOT0..2 and relies on them starting at zero
  DPO_CHECK(hipMemset(c->ctrl, 0, CTRL_SIZE * sizeof(double)));
  DPO_CHECK(hipMalloc(&c->G_buf, vb));
  // delta is consumed as `beta*delta - z` with beta == 0 on the first
  // tCG iteration: one-time zeroing keeps 0*garbage (possible NaN bit
  // patterns in fresh allocations) out of the recurrence, and the
  // per-solve zeroing passes are dropped from the captured body
  DPO_CHECK(hipMemset(c->delta, 0, vb));
  DPO_CHECK(hipMemset(c->delta1, 0, vb));  // the "old" buffer of iteration 0
  DPO_CHECK(hipMemset(c->eta, 0, vb));
  DPO_CHECK(hipHostMalloc(&c->ctrl_host, CTRL_SIZE * sizeof(double)));
  DPO_CHECK(hipHostGetDevicePointer((void**)&c->ctrl_host_dev,
                                    c->ctrl_host, 0));
  DPO_CHECK(hipStreamCreateWithFlags(&c->cap_stream,
                                     hipStreamNonBlocking));
  DPO_CHECK(hipStreamCreateWithFlags(&c->exec_stream,
                                     hipStreamNonBlocking));
  DPO_CHECK(hipEventCreateWithFlags(&c->start_event,
                                    hipEventDisableTiming));
  DPO_CHECK(hipEventCreateWithFlags(&c->done_event,
                                    hipEventDisableTiming));
  DPO_CHECK(hipMalloc(&c->fences, F_NUM * sizeof(unsigned int)));
  DPO_CHECK(hipMemset(c->fences, 0, F_NUM * sizeof(unsigned int)));
  DPO_CHECK(hipMalloc(&c->eval3, 3 * sizeof(double)));
  return c;
}

void dpo_ctx_destroy(void* h) {
  DpoCtx* c = (DpoCtx*)h;
  dpo_ignore(hipFree(c->W)); dpo_ignore(hipFree(c->grad)); dpo_ignore(hipFree(c->eta)); dpo_ignore(hipFree(c->delta)); dpo_ignore(hipFree(c->delta1));
  dpo_ignore(hipFree(c->rvec)); dpo_ignore(hipFree(c->z)); dpo_ignore(hipFree(c->Hd)); dpo_ignore(hipFree(c->step));
  dpo_ignore(hipFree(c->Xprop)); dpo_ignore(hipFree(c->eta_snap)); dpo_ignore(hipFree(c->delta_snap));
  c->invalidate_graphs();
  if (c->cap_stream) dpo_ignore(hipStreamDestroy(c->cap_stream));
  if (c->exec_stream) dpo_ignore(hipStreamDestroy(c->exec_stream));
  if (c->start_event) dpo_ignore(hipEventDestroy(c->start_event));
  if (c->done_event) dpo_ignore(hipEventDestroy(c->done_event));
  dpo_ignore(hipFree(c->ctrl)); dpo_ignore(hipFree(c->G_buf)); dpo_ignore(hipHostFree(c->ctrl_host));
  dpo_ignore(hipFree(c->fences)); dpo_ignore(hipFree(c->eval3));
  delete c;
}

void dpo_ctx_set_problem(void* h, const int* rp, const int* ci,
                         const double* vals, const double* Gt,
                         const float* Minv, const double* Ljac) {
  DpoCtx* c = (DpoCtx*)h;
  if (c->q_vals != vals || c->Minv != Minv || c->Ljac != Ljac
      || c->Gt != Gt || c->q_rp != rp)
    c->invalidate_graphs();
  if (c->q_vals != vals || c->Minv != Minv || c->Ljac != Ljac
      || c->q_rp != rp || c->q_ci != ci)
    c->desc_stamp++;
  c->q_rp = rp; c->q_ci = ci; c->q_vals = vals;
  c->Gt = Gt; c->Minv = Minv; c->Ljac = Ljac;
}

}  // extern "C"

// DPO_TCG_SEG=K: tCG iterations in the primary solve graph. The solve
// graph is static, so every iteration it holds is launched whether or
// not tCG has already stopped (a stopped iteration is 5-6 guarded no-op
// launches at the dispatch floor each). With K < max_inner the primary
// graph holds only K iterations; the rare solve still running after
// them gets the rest from a second (continuation) graph, launched by
// the host after the sync it performs anyway. 0 or >= max_inner: one
// graph with every iteration. Unset: 3 with the dense preconditioner
// (small, launch-bound agents: tCG stops after 2-4 iterations), one
// graph with block-Jacobi (large agents: tCG usually runs to the cap,
// so nearly every solve would continue). Both from the measured
// iteration histograms, docs/DESIGN.md section 3.
#define DPO_TCG_SEG_DENSE 3
static int solve_segment(const DpoCtx* c) {
  static const int env = [] {
    const char* v = getenv("DPO_TCG_SEG");
    return v ? atoi(v) : -1;
  }();
  const int seg = env >= 0 ? env : (c->Minv ? DPO_TCG_SEG_DENSE : 0);
  return (seg <= 0 || seg >= c->max_inner) ? c->max_inner : seg;
}

// The solve sequence (gradient, tCG, first candidate + acceptance test)
// in three pieces; every operand pointer is stable across rounds by
// construction, so any concatenation of them is capturable as a
// hipGraph.
//
// Fused control tails (CF_*): the tCG scalar decisions run in the
// last-arriving block of the producing reduction kernel instead of a
// dedicated single-wave kernel, removing 3 of 8 launches per tCG
// iteration. The ~4 us/launch dispatch latency floor is what bounds
// these small-agent solves (see profiles/), so launch count is the
// lever. An earlier attempt at this fusion showed trajectory scatter
// that was eventually root-caused to an LDS reuse race in
// block_reduce_atomic plus the hipGraph ordering bugs (both fixed);
// DPO_NO_CF=1 runs each tail as a standalone k_ctrl_tail launch.
static bool solve_no_cf() {
  static const bool no_cf = dpo_env_flag("DPO_NO_CF");
  return no_cf;
}

// One reduction stage of the solve: launch(cf) enqueues its kernel with
// the control tail cf (an integral_constant) fused in — the stage's own
// tail CF by default; with DPO_NO_CF=1, CF_NONE followed by the tail's
// standalone launch.
template <int CF, class Launch>
static void enqueue_with_tail(DpoCtx* c, hipStream_t s, Launch launch) {
  if (solve_no_cf()) {
    launch(std::integral_constant<int, CF_NONE>{});
    launch_ctrl_tail<CF>(c->ctrl, s);
  } else {
    launch(std::integral_constant<int, CF>{});
  }
}

// Hd stage: Hd = P_X(Q delta), <delta, Hd>, alpha / boundary decision.
// Folded (default): the direction update delta = beta * delta - z rides
// in the same kernel (AUX = 2, double-buffered delta). Otherwise
// k_tcg_delta has run behind the z stage, in place on buffer 0.
// Folded with the dense preconditioner only, the small launch-bound
// agents (same split as DPO_TCG_SEG_DENSE): with block-Jacobi at 125k
// poses per agent the kernel's doubled neighbour loads cost more than the
// launch saves (1M-pose round 11.05 -> 11.62 ms, RESULTS.md).
// The fusions of this file's newer tails (CF_INIT, k_candidate,
// CF_ACCEPT*, CF_EVAL, the folded Hd stage) serve the small, launch-bound
// agents, which are the ones that use the dense preconditioner (the same
// split as DPO_TCG_SEG_DENSE). With block-Jacobi at 125k poses per agent
// a launch is noise and the fan-in of ~500 blocks per tail is not: the
// 1M-pose round was 0.7 to 1 % slower with them in nine of nine pairs
// (RESULTS.md), so that path keeps the standalone launches.
static bool ctx_fuse_scalar(const DpoCtx* c) {
  return c->Minv && !solve_no_cf();
}

// The folded Hd stage on raw pointers (solve body and dpo_hd_stage).
static void launch_hd_folded(const int* rp, const int* ci,
                             const double* vals, double* d0, double* d1,
                             const double* z, const double* X, double* Hd,
                             double* ctrl, int n, int d, int r,
                             hipStream_t s) {
  launch_hess_fused<0, CF_ALPHA, 2>(rp, ci, vals, nullptr, X, nullptr, Hd, z,
                                    ctrl, n, d, r, C_DOT0, -1, ST_RUN, s, -1,
                                    d1, d0);
}

static bool ctx_fold_delta(const DpoCtx* c) {
  return ctx_fuse_scalar(c) && !hess_use_wide(c->n);
}

static void enqueue_hd_stage(DpoCtx* c, const double* X, hipStream_t s) {
  if (ctx_fold_delta(c)) {
    launch_hd_folded(c->q_rp, c->q_ci, c->q_vals, c->delta, c->delta1, c->z,
                     X, c->Hd, c->ctrl, c->n, c->d, c->r, s);
    return;
  }
  enqueue_with_tail<CF_ALPHA>(c, s, [&](auto cf) {
    ctx_hess<0, cf>(c, c->delta, X, nullptr, c->Hd, c->delta, C_DOT0, -1,
                    ST_RUN, s);
  });
}

// Update stage: snapshots, eta and residual updates, ||r||^2, stop test.
// Clears ctx_prezero_z(c) for the dense apply of the z stage behind it.
static void enqueue_update_stage(DpoCtx* c, hipStream_t s) {
  enqueue_with_tail<CF_RR>(c, s, [&](auto cf) {
    launch_tcg_update<cf>(c->eta, c->rvec, c->delta, c->Hd, c->eta_snap,
                          c->delta_snap, c->ctrl, c->total,
                          ctx_prezero_z(c), s,
                          ctx_fold_delta(c) ? c->delta1 : nullptr);
  });
}

// z stage: z = P_X(M^-1 r), <z, r>, then the tail CF (CF_Z0 for z0,
// CF_BETA in the loop). Block-Jacobi (large agents) does all of it in
// one k_precond_proj launch; the dense apply runs standalone in front of
// the projection kernel, and so does the Jacobi apply under DPO_NO_CF=1.
template <int CF>
static void enqueue_z_stage(DpoCtx* c, const double* X, hipStream_t s) {
  if (!c->Minv && !solve_no_cf()) {
    if (!dispatch_dr(c->d, c->r, [&](auto Dc, auto Rc) {
          hipLaunchKernelGGL((k_precond_proj<Dc, Rc, CF>),
                             dim3(blocks_for(c->n, 256)), dim3(256), 0, s,
                             c->Ljac, c->rvec, X, c->z, c->ctrl, c->n,
                             C_DOT0, ST_RUN);
        }))
      dpo_bad_shape(c->d, c->r);
    return;
  }
  ctx_precond(c, c->rvec, c->z, s);
  enqueue_with_tail<CF>(c, s, [&](auto cf) {
    launch_proj_dots<cf>(X, c->z, nullptr, c->z, c->rvec, c->ctrl, c->n,
                         c->d, c->r, C_DOT0, -1, ST_RUN, s);
  });
}

// Head: G assembly, gradient, control init, z0 and the first delta.
static void enqueue_solve_head(DpoCtx* c, double* X, const double* nbr,
                               double tol, double Delta0, hipStream_t s) {
  fence_wait(c, F_SOLVE_IN, s);  // first node: block until inputs ready
  // fused (default): G_buf and the control block cleared by one launch,
  // the control init run by the gradient kernel's last block
  const bool fused = ctx_fuse_scalar(c);
  if (nbr) ctx_assemble_g(c, nbr, s, /*with_ctrl=*/fused);
  if (!nbr || !fused) dzero(c->ctrl, CTRL_SIZE, s);

  // gradient phase: one fused kernel computes Q@X + G, projects at X
  // and accumulates <P,P> / <QX+G,X> (was spmm + proj_dots — the
  // two-kernel split re-read the full iterate from HBM). It writes the
  // gradient to grad and to rvec (the tCG residual starts as the
  // gradient) and clears z for the z0 dense apply.
  if (fused) {
    TailArgs ta;
    ta.a = tol; ta.b = Delta0; ta.c = 1.0; ta.d = 0.1;
    ctx_hess<0, CF_INIT, 1>(c, X, X, c->Gt, c->grad, nullptr, C_DOT1, C_DOT0,
                            -1, s, c->Gt ? C_DOT2 : -1, c->rvec,
                            ctx_prezero_z(c), ta);
  } else {
    ctx_hess<0, CF_NONE, 1>(c, X, X, c->Gt, c->grad, nullptr, C_DOT1,
                            C_DOT0, -1, s,
                            c->Gt ? C_DOT2 : -1,  // <G,X> folded in
                            c->rvec, ctx_prezero_z(c));
    dpo_ctrl_init(c->ctrl, tol, Delta0, 1.0, 0.1, s);
  }
  enqueue_z_stage<CF_Z0>(c, X, s);
  if (!ctx_fold_delta(c)) dpo_tcg_delta(c->delta, c->z, c->ctrl, c->total, s);
}

// `count` tCG iterations. Position-independent: every kernel reads the
// iteration index from the control block (C_ITER) and is a no-op unless
// the status is ST_RUN.
static void enqueue_tcg_iters(DpoCtx* c, double* X, int count,
                              hipStream_t s) {
  for (int j = 0; j < count; ++j) {
    enqueue_hd_stage(c, X, s);
    enqueue_update_stage(c, s);
    enqueue_z_stage<CF_BETA>(c, X, s);
    if (!ctx_fold_delta(c))
      dpo_tcg_delta(c->delta, c->z, c->ctrl, c->total, s);
  }
}

// One trust-region candidate at the current radius: pick the step from
// the stored Krylov path, retract, evaluate f, run the acceptance test.
// Every kernel is guarded by ST_TCG_STOP.
//
// Fused (default): two launches, k_candidate and the f evaluation whose
// last block runs the acceptance test. With publish (end of a solve
// sequence) that kernel also copies the control block to the host and
// releases F_SOLVE_OUT; it then is the sequence's last node. DPO_NO_CF=1:
// the five standalone launches, and publishing is left to the caller.
static void launch_candidate(double* ctrl, double* step, const double* eta,
                             const double* eta_snap,
                             const double* delta_snap, const double* X,
                             double* Xprop, int n, int d, int r,
                             hipStream_t s) {
  if (!dispatch_dr(d, r, [&](auto Dc, auto Rc) {
        hipLaunchKernelGGL((k_candidate<Dc, Rc>), dim3(blocks_for(n, 256)),
                           dim3(256), 0, s, ctrl, step, eta, eta_snap,
                           delta_snap, X, Xprop, n);
      }))
    dpo_bad_shape(d, r);
}

static void enqueue_candidate(DpoCtx* c, const double* X, double accept_rho,
                              hipStream_t s, bool publish = false) {
  if (!ctx_fuse_scalar(c)) {
    dpo_ctrl_candidate(c->ctrl, s);
    dpo_form_step(c->step, c->eta, c->eta_snap, c->delta_snap, c->ctrl,
                  c->total, s);
    launch_polar(X, c->step, nullptr, 1.0, 1.0, 0.0, c->Xprop, c->n, c->d,
                 c->r, c->ctrl, ST_TCG_STOP, s);
    ctx_hess<1>(c, c->Xprop, nullptr, c->Gt, nullptr, nullptr, C_DOT0,
                C_DOT2, ST_TCG_STOP, s);
    dpo_ctrl_accept(c->ctrl, accept_rho, s);
    return;
  }
  launch_candidate(c->ctrl, c->step, c->eta, c->eta_snap, c->delta_snap, X,
                   c->Xprop, c->n, c->d, c->r, s);
  TailArgs ta;
  ta.a = accept_rho;
  if (publish) {
    ta.dst = c->ctrl_host_dev;
    ta.fence = c->fences + F_SOLVE_OUT;
    ctx_hess<1, CF_ACCEPT_OUT>(c, c->Xprop, nullptr, c->Gt, nullptr, nullptr,
                               C_DOT0, C_DOT2, ST_TCG_STOP, s, -1, nullptr,
                               nullptr, ta);
  } else {
    ctx_hess<1, CF_ACCEPT>(c, c->Xprop, nullptr, c->Gt, nullptr, nullptr,
                           C_DOT0, C_DOT2, ST_TCG_STOP, s, -1, nullptr,
                           nullptr, ta);
  }
}

static void ctx_ctrl_to_host(DpoCtx* c, hipStream_t s) {
  hipLaunchKernelGGL(k_ctrl_to_host, dim3(1), dim3(64), 0, s, c->ctrl,
                     c->ctrl_host_dev, CTRL_SIZE);
}

// Tail: first candidate + acceptance test, control block to the host.
// Behind a segment that left tCG running the candidate is a no-op and
// the host reads ST_RUN.
static void enqueue_solve_tail(DpoCtx* c, double* X, double accept_rho,
                               hipStream_t s) {
  enqueue_candidate(c, X, accept_rho, s, /*publish=*/true);
  if (!ctx_fuse_scalar(c)) {
    ctx_ctrl_to_host(c, s);
    fence_signal(c, F_SOLVE_OUT, s);  // last node: mark sequence complete
  }
}

// Primary sequence: head + `iters` tCG iterations + tail. The max_inner
// cap (k_ctrl_tcg_end) belongs to the segment that holds the last
// iteration.
static void enqueue_solve_body(DpoCtx* c, double* X, const double* nbr,
                               double tol, double Delta0,
                               double accept_rho, int iters,
                               hipStream_t s) {
  enqueue_solve_head(c, X, nbr, tol, Delta0, s);
  enqueue_tcg_iters(c, X, iters, s);
  if (iters >= c->max_inner) dpo_ctrl_tcg_end(c->ctrl, s);
  enqueue_solve_tail(c, X, accept_rho, s);
}

// Continuation sequence: the iterations after the primary's `done`.
static void enqueue_solve_cont(DpoCtx* c, double* X, double accept_rho,
                               int done, hipStream_t s) {
  fence_wait(c, F_SOLVE_IN, s);
  enqueue_tcg_iters(c, X, c->max_inner - done, s);
  dpo_ctrl_tcg_end(c->ctrl, s);
  enqueue_solve_tail(c, X, accept_rho, s);
}

static inline const void* solve_key_scalars(double tol, double accept_rho) {
  return (const void*)((intptr_t)(tol * 1e9)
                       ^ ((intptr_t)(accept_rho * 1e6) << 36));
}

// Ensure the solve graph for (X, nbr, tol, Delta0) is cached; run the
// pre-sync sequence (via graph replay or eagerly) on stream s WITHOUT
// the final synchronize. Returns true when the sequence was enqueued
// asynchronously (graph path) — eager fallback syncs internally.
static bool solve_presync(DpoCtx* c, double* X, const double* nbr,
                          double tol, double Delta0, double accept_rho,
                          hipStream_t s) {
  static const bool no_graph = dpo_env_flag("DPO_NO_SOLVE_GRAPH");
  // the eager paths enqueue every iteration: nothing is saved by
  // segmenting a sequence that is not replayed
  if (no_graph) {
    // fully async eager enqueue; callers sync (finish / impl)
    enqueue_solve_body(c, X, nbr, tol, Delta0, accept_rho, c->max_inner,
                       s);
    fence_wait(c, F_SOLVE_OUT, s);
    return true;
  }
  // accept_rho is an argument of the captured acceptance test too: it
  // shares a key slot with tol
  const void* key[4] = {X, nbr, solve_key_scalars(tol, accept_rho),
                        (const void*)(intptr_t)Delta0};
  const int seg = solve_segment(c);
  const bool launched = graph_cache_launch(
      c->solve_graph, key, c->cap_stream, s, [&](hipStream_t cs) {
        enqueue_solve_body(c, X, nbr, tol, Delta0, accept_rho, seg, cs);
      });
  if (!launched) {
    // capture unavailable: run eagerly on the caller's stream
    enqueue_solve_body(c, X, nbr, tol, Delta0, accept_rho, c->max_inner,
                       s);
    fence_wait(c, F_SOLVE_OUT, s);
    DPO_CHECK(hipStreamSynchronize(s));
    return false;
  }
  // eager wait pins downstream stream work (and host syncs) to the
  // graph's actual completion even if the launch misordered
  fence_wait(c, F_SOLVE_OUT, s);
  return true;
}

// After the primary sequence has completed on s (ctrl_host is valid):
// if it left tCG running — only a primary graph shorter than max_inner
// can — launch the continuation graph on s, fenced like the primary,
// and return true; the caller syncs s again before solve_postsync.
static bool solve_continue(DpoCtx* c, double* X, const double* nbr,
                           double tol, double Delta0, double accept_rho,
                           hipStream_t s) {
  if ((int)c->ctrl_host[C_STATUS] != ST_RUN) return false;
  const int seg = solve_segment(c);
  if (seg >= c->max_inner) return false;
  c->n_conts++;
  fence_signal(c, F_SOLVE_IN, s);
  // accept_rho is an argument of the captured acceptance test too: it
  // shares a key slot with tol
  const void* key[4] = {X, nbr, solve_key_scalars(tol, accept_rho),
                        (const void*)(intptr_t)Delta0};
  const bool launched = graph_cache_launch(
      c->cont_graph, key, c->cap_stream, s, [&](hipStream_t cs) {
        enqueue_solve_cont(c, X, accept_rho, seg, cs);
      });
  if (!launched) enqueue_solve_cont(c, X, accept_rho, seg, s);
  fence_wait(c, F_SOLVE_OUT, s);
  return true;
}

// Post-sync part of the solve: acceptance decision + (rare) shrink
// loop. Assumes the pre-sync sequence has completed on stream s and
// ctrl_host holds the control block. A rejected first candidate
// enqueues the ENTIRE guarded radius-shrink loop in one batch (each
// attempt's kernels no-op via the ctrl guard once a candidate is
// accepted) behind a single stream sync, instead of a host round-trip
// per attempt.
// commit == false leaves X <- Xprop of an accepted step to the caller
// (the batched finish commits every member with one launch).
static int solve_postsync(DpoCtx* c, double* X, double accept_rho,
                          int max_shrink, int compute_final_gn,
                          double* stats_out, hipStream_t s,
                          bool commit = true) {
  int st = (int)c->ctrl_host[C_STATUS];
  if (st == ST_TCG_STOP && max_shrink > 0) {
    for (int attempt = 1; attempt <= max_shrink; ++attempt) {
      dpo_ctrl_shrink(c->ctrl, s);
      enqueue_candidate(c, X, accept_rho, s);
    }
    ctx_ctrl_to_host(c, s);
    DPO_CHECK(hipStreamSynchronize(s));
    st = (int)c->ctrl_host[C_STATUS];
  }
  const int shrinks = (int)c->ctrl_host[C_SHRINKS];
  int status = st;
  if (st == ST_ACCEPTED) {
    if (commit)
      DPO_CHECK(hipMemcpyAsync(X, c->Xprop, c->total * sizeof(double),
                               hipMemcpyDeviceToDevice, s));
  } else if (st == ST_TCG_STOP) {
    status = ST_GIVE_UP;  // every radius rejected: keep the iterate
  }

  double f_init = c->ctrl_host[C_FX];
  double gn_init = sqrt(c->ctrl_host[C_GN0SQ]);
  double f_opt = (status == ST_ACCEPTED) ? c->ctrl_host[C_FPROP] : f_init;
  double gn_opt = gn_init;
  if (compute_final_gn && status == ST_ACCEPTED) {
    DPO_CHECK(hipMemsetAsync(c->ctrl + C_DOT1, 0, sizeof(double), s));
    ctx_hess<0>(c, X, X, c->Gt, c->grad, nullptr, C_DOT1, -1, -1, s);
    DPO_CHECK(hipMemcpyAsync(c->ctrl_host + C_DOT1, c->ctrl + C_DOT1,
                             sizeof(double), hipMemcpyDeviceToHost, s));
    DPO_CHECK(hipStreamSynchronize(s));
    gn_opt = sqrt(c->ctrl_host[C_DOT1]);
  }
  c->n_solves++;
  {
    const int hlen = (int)c->ctrl_host[C_HLEN];
    c->hlen_hist[hlen < 0 ? 0 : (hlen > MAX_TCG ? MAX_TCG : hlen)]++;
  }
  if (stats_out) {
    stats_out[0] = status;
    stats_out[1] = f_init;
    stats_out[2] = gn_init;
    stats_out[3] = f_opt;
    stats_out[4] = gn_opt;
    stats_out[5] = c->ctrl_host[C_RHO];
    stats_out[6] = shrinks;
    stats_out[7] = c->ctrl_host[C_HLEN];
  }
  return status;
}

// Full RBCD local solve in place on X. stats_out (host, >= 8 doubles):
// [status, f_init, gn_init, f_opt, gn_opt, rho, shrink_count, hlen].
// nbr != null: assemble G from the packed neighbor buffer first; the
// whole pre-sync sequence is then served from a cached hipGraph.
static int rbcd_solve_impl(DpoCtx* c, double* X, const double* nbr,
                           double tol, double Delta0, int max_shrink,
                           double accept_rho, int compute_final_gn,
                           double* stats_out, hipStream_t s) {
  fence_signal(c, F_SOLVE_IN, s);
  bool async = solve_presync(c, X, nbr, tol, Delta0, accept_rho, s);
  if (async) DPO_CHECK(hipStreamSynchronize(s));
  if (solve_continue(c, X, nbr, tol, Delta0, accept_rho, s))
    DPO_CHECK(hipStreamSynchronize(s));
  return solve_postsync(c, X, accept_rho, max_shrink, compute_final_gn,
                        stats_out, s);
}

extern "C" {

int dpo_rbcd_solve(void* h, double* X, double tol, double Delta0,
                   int max_shrink, double accept_rho,
                   int compute_final_gn, double* stats_out, void* stream) {
  return rbcd_solve_impl((DpoCtx*)h, X, nullptr, tol, Delta0, max_shrink,
                         accept_rho, compute_final_gn, stats_out,
                         (hipStream_t)stream);
}

// --- async (multi-stream) round entry points ------------------------
// Launch the solve's pre-sync sequence on the ctx's private execution
// stream, ordered after the caller's stream. Finish with
// dpo_round_solve_finish. Concurrent agents overlap on the GPU.
void dpo_round_solve_async(void* h, double* X, const double* nbr,
                           double tol, double Delta0, double accept_rho,
                           void* join_stream) {
  DpoCtx* c = (DpoCtx*)h;
  hipStream_t js = (hipStream_t)join_stream;
  // the IN fence is signalled on the PRODUCER (torch) stream: it
  // carries the completion of the boundary-pose scatter into the solve
  // sequence as a data dependency (see fence comment above). No event
  // ceremony — the fence IS the ordering mechanism (launch-order
  // hipStreamWaitEvent is exactly what graph launches fail to honor).
  fence_signal(c, F_SOLVE_IN, js);
  solve_presync(c, X, nbr, tol, Delta0, accept_rho, c->exec_stream);
  c->pend_X = X;
  c->pend_nbr = nbr;
  c->pend_tol = tol;
  c->pend_Delta0 = Delta0;
  c->pend_rho = accept_rho;
}

// Finishing an async solve takes two steps, so that a group can run
// step 1 for every agent before step 2 for any: one agent's
// continuation then overlaps the others' instead of serialising them.
// Step 1: wait for the primary sequence; launch the continuation if
// tCG is still running. Returns whether it did.
static bool round_finish_primary(DpoCtx* c) {
  DPO_CHECK(hipStreamSynchronize(c->exec_stream));
  return solve_continue(c, c->pend_X, c->pend_nbr, c->pend_tol,
                        c->pend_Delta0, c->pend_rho, c->exec_stream);
}

// Step 2: wait for the continuation (if any), post-process, join.
static int round_finish_post(DpoCtx* c, bool continued, int max_shrink,
                             double* stats_out, hipStream_t js) {
  if (continued) DPO_CHECK(hipStreamSynchronize(c->exec_stream));
  int st = solve_postsync(c, c->pend_X, c->pend_rho, max_shrink, 0,
                          stats_out, c->exec_stream);
  DPO_CHECK(hipEventRecord(c->done_event, c->exec_stream));
  DPO_CHECK(hipStreamWaitEvent(js, c->done_event, 0));
  return st;
}

int dpo_round_solve_finish(void* h, int max_shrink, double* stats_out,
                           void* join_stream) {
  DpoCtx* c = (DpoCtx*)h;
  const bool continued = round_finish_primary(c);
  return round_finish_post(c, continued, max_shrink, stats_out,
                           (hipStream_t)join_stream);
}

// The device control block, copied out synchronously (tests: every slot,
// where the host copy a solve publishes may be a prefix). Writes at
// most `cap` slots; returns CTRL_SIZE.
int dpo_ctx_ctrl(void* h, double* out, int cap) {
  DpoCtx* c = (DpoCtx*)h;
  const int m = cap < CTRL_SIZE ? cap : CTRL_SIZE;
  DPO_CHECK(hipDeviceSynchronize());
  DPO_CHECK(hipMemcpy(out, c->ctrl, m * sizeof(double),
                      hipMemcpyDeviceToHost));
  return CTRL_SIZE;
}

// --- the fused stages as stand-alone ops (tests) ---------------------
// k_candidate on caller-owned buffers; equals dpo_ctrl_candidate +
// dpo_form_step + dpo_polar_affine(X, step, 1, 1, guard ST_TCG_STOP).
void dpo_candidate(double* ctrl, double* step, const double* eta,
                   const double* eta_snap, const double* delta_snap,
                   const double* X, double* Xprop, int n, int d, int r,
                   void* stream) {
  launch_candidate(ctrl, step, eta, eta_snap, delta_snap, X, Xprop, n, d, r,
                   (hipStream_t)stream);
}

// One Hessian stage with its scalar step, fused into the kernel's last
// block (fused != 0) or as the launch of its own that DPO_NO_CF=1 runs.
//   kind 1  solve head: out = grad, out2 = its copy, then the control
//           init with tol = a, Delta0 = b (theta = 1, kappa = 0.1)
//   kind 2  candidate evaluation of V (guard ST_TCG_STOP), then the
//           acceptance test with accept_rho = a
//   kind 3  evaluation: out = grad, then out3[0..2] and the dot clean-up
void dpo_hess_tail(const int* rp, const int* ci, const double* vals,
                   const double* V, const double* G, double* out,
                   double* out2, double* ctrl, int n, int d, int r,
                   int kind, int fused, double a, double b, double* out3,
                   void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int s3 = G ? C_DOT2 : -1;
  TailArgs ta;
  ta.a = a; ta.b = b; ta.c = 1.0; ta.d = 0.1; ta.dst = out3;
  if (kind == 1) {
    if (fused) {
      launch_hess_fused<0, CF_INIT, 1>(rp, ci, vals, V, V, G, out, nullptr,
                                       ctrl, n, d, r, C_DOT1, C_DOT0, -1, s,
                                       s3, out2, nullptr, ta);
    } else {
      launch_hess_fused<0, CF_NONE, 1>(rp, ci, vals, V, V, G, out, nullptr,
                                       ctrl, n, d, r, C_DOT1, C_DOT0, -1, s,
                                       s3, out2, nullptr);
      dpo_ctrl_init(ctrl, a, b, 1.0, 0.1, stream);
    }
  } else if (kind == 2) {
    if (fused) {
      launch_hess_fused<1, CF_ACCEPT>(rp, ci, vals, V, nullptr, G, nullptr,
                                      nullptr, ctrl, n, d, r, C_DOT0, C_DOT2,
                                      ST_TCG_STOP, s, -1, nullptr, nullptr,
                                      ta);
    } else {
      launch_hess_fused<1>(rp, ci, vals, V, nullptr, G, nullptr, nullptr,
                           ctrl, n, d, r, C_DOT0, C_DOT2, ST_TCG_STOP, s);
      dpo_ctrl_accept(ctrl, a, stream);
    }
  } else if (kind == 3) {
    if (fused) {
      launch_hess_fused<0, CF_EVAL>(rp, ci, vals, V, V, G, out, nullptr,
                                    ctrl, n, d, r, C_DOT1, C_DOT0, -1, s, s3,
                                    nullptr, nullptr, ta);
    } else {
      launch_hess_fused<0>(rp, ci, vals, V, V, G, out, nullptr, ctrl, n, d,
                           r, C_DOT1, C_DOT0, -1, s, s3);
      hipLaunchKernelGGL(k_eval_combine, dim3(1), dim3(64), 0, s, ctrl,
                         out3);
    }
  } else {
    fprintf(stderr, "dpo_hess_tail: unknown kind %d\n", kind);
    abort();
  }
}

// The tCG Hd stage on caller-owned buffers: Hd = P_X(Q delta) with
// delta = C_BETA * delta_old - z, <delta, Hd> and the alpha tail (status
// ST_RUN only). fused != 0: one kernel, delta_old read from buffer
// 1 - (C_ITER & 1) of (d0, d1) and delta written to the other.
// fused == 0: k_tcg_delta in place on d0, then the Hessian kernel on it.
void dpo_hd_stage(const int* rp, const int* ci, const double* vals,
                  double* d0, double* d1, const double* z, const double* X,
                  double* Hd, double* ctrl, int n, int d, int r, int fused,
                  void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (fused) {
    launch_hd_folded(rp, ci, vals, d0, d1, z, X, Hd, ctrl, n, d, r, s);
  } else {
    dpo_tcg_delta(d0, z, ctrl, (long)n * (d + 1) * r, stream);
    launch_hess_fused<0, CF_ALPHA>(rp, ci, vals, d0, X, nullptr, Hd, d0,
                                   ctrl, n, d, r, C_DOT0, -1, ST_RUN, s);
  }
}

// tCG iterations in the primary solve graph of this context, for the
// problem currently bound (DPO_TCG_SEG resolved); == max_inner: one graph.
int dpo_tcg_segment(void* h) { return solve_segment((DpoCtx*)h); }

// out[0] = solves, out[1] = continuation launches, out[2 + h] = solves
// that ended with C_HLEN == h (h = 0 .. MAX_TCG). Writes at most `cap`
// entries; returns the full length.
int dpo_ctx_counters(void* h, long* out, int cap) {
  DpoCtx* c = (DpoCtx*)h;
  const int len = 2 + MAX_TCG + 1;
  for (int i = 0; i < len && i < cap; ++i)
    out[i] = (i == 0) ? c->n_solves
           : (i == 1) ? c->n_conts : c->hlen_hist[i - 2];
  return len;
}

}  // extern "C"

// The evaluation's kernels. Fused (default): the gradient kernel's last
// block writes the three scalars, cleans the dot slots and, with a
// fence, releases it. DPO_NO_CF=1: k_eval_combine, and k_fence_signal
// for the fence, as launches of their own.
static void eval_terms(DpoCtx* c, const double* X, double* out_dev,
                       hipStream_t s, unsigned int* fence) {
  if (!ctx_fuse_scalar(c)) {
    ctx_hess<0>(c, X, X, c->Gt, c->grad, nullptr, C_DOT1, C_DOT0, -1, s,
                c->Gt ? C_DOT2 : -1);
    hipLaunchKernelGGL(k_eval_combine, dim3(1), dim3(64), 0, s, c->ctrl,
                       out_dev);
    if (fence)
      hipLaunchKernelGGL(k_fence_signal, dim3(1), dim3(64), 0, s, fence);
    return;
  }
  TailArgs ta;
  ta.dst = out_dev;
  ta.fence = fence;
  ctx_hess<0, CF_EVAL>(c, X, X, c->Gt, c->grad, nullptr, C_DOT1, C_DOT0, -1,
                       s, c->Gt ? C_DOT2 : -1, nullptr, nullptr, ta);
}

extern "C" {

// Per-round evaluation: out_dev (>=3 doubles, device) = [f, 0.5<X,G>, gn2]
// using the ctx's problem pointers. No host sync.
void dpo_eval_terms(void* h, const double* X, double* out_dev,
                    void* stream) {
  DpoCtx* c = (DpoCtx*)h;
  hipStream_t s = (hipStream_t)stream;
  // dot slots are pre-zeroed (zero-init at allocation; k_eval_combine
  // self-cleans after each eval; solves wipe the whole control block)
  // ONE fused kernel: Q@X + G, projection at X, and all three scalars
  // <P,P> / <QX+G,X> / <G,X> (the standalone <G,X> k_dots re-read
  // 2x the iterate from HBM and was the eval phase's fattest kernel
  // at 1M poses — profiles/r2c_narrow)
  eval_terms(c, X, out_dev, s, nullptr);
}


// Install the static G-assembly structure (per-agent, set once; weights
// pointer re-read every assembly so GNC re-weighting is free).
void dpo_ctx_set_gdata(void* h, const double* E0, const long* local_pose,
                       const long* nbr_slot, const double* w, int ne) {
  DpoCtx* c = (DpoCtx*)h;
  if (c->g_E0 != E0 || c->g_w != w) c->invalidate_graphs();
  if (c->g_E0 != E0 || c->g_w != w || c->g_local_pose != local_pose
      || c->g_nbr_slot != nbr_slot || c->g_ne != ne)
    c->desc_stamp++;
  c->g_E0 = E0; c->g_local_pose = local_pose; c->g_nbr_slot = nbr_slot;
  c->g_w = w; c->g_ne = ne;
}

// Fused per-round entry points: assemble G from the packed neighbor
// buffer, then solve / evaluate. One Python call each.
int dpo_round_solve(void* h, double* X, const double* nbr, double tol,
                    double Delta0, int max_shrink, double accept_rho,
                    double* stats_out, void* stream) {
  return rbcd_solve_impl((DpoCtx*)h, X, nbr, tol, Delta0, max_shrink,
                         accept_rho, 0, stats_out, (hipStream_t)stream);
}

// Fenced eval body: wait on the IN fence, assemble G + evaluate, signal
// the OUT fence. Used for both capture and eager enqueue.
static void enqueue_eval_body(DpoCtx* c, const double* X, const double* nbr,
                              double* out_dev, hipStream_t s) {
  fence_wait(c, F_EVAL_IN, s);
  ctx_assemble_g(c, nbr, s);
  // the OUT fence is released by the evaluation's last kernel
  eval_terms(c, X, out_dev, s, c->fences + F_EVAL_OUT);
}

// IN fence must already be signalled on the producer stream. With
// wait_out=false the caller consumes the OUT fence itself (group
// fan-out path: one gather kernel waits on every agent's OUT fence).
static void round_eval_impl(DpoCtx* c, const double* X, const double* nbr,
                            double* out_dev, hipStream_t s,
                            bool wait_out = true) {
  static const bool no_graph = dpo_env_flag("DPO_NO_EVAL_GRAPH");
  if (no_graph) {
    enqueue_eval_body(c, X, nbr, out_dev, s);
    if (wait_out) fence_wait(c, F_EVAL_OUT, s);
    return;
  }
  const void* key[4] = {X, nbr, out_dev, nullptr};
  const bool launched = graph_cache_launch(
      c->eval_graph, key, c->cap_stream, s, [&](hipStream_t cs) {
        enqueue_eval_body(c, X, nbr, out_dev, cs);
      });
  // capture unavailable: run eagerly on the caller's stream
  if (!launched) enqueue_eval_body(c, X, nbr, out_dev, s);
  if (wait_out) fence_wait(c, F_EVAL_OUT, s);
}

void dpo_round_eval(void* h, const double* X, const double* nbr,
                    double* out_dev, void* stream) {
  DpoCtx* c = (DpoCtx*)h;
  hipStream_t s = (hipStream_t)stream;
  fence_signal(c, F_EVAL_IN, s);
  round_eval_impl(c, X, nbr, out_dev, s);
}

void dpo_round_eval_async(void* h, const double* X, const double* nbr,
                          double* out_dev, void* join_stream) {
  DpoCtx* c = (DpoCtx*)h;
  hipStream_t js = (hipStream_t)join_stream;
  // IN fence on the producer stream: carries the boundary-pose scatter
  fence_signal(c, F_EVAL_IN, js);
  round_eval_impl(c, X, nbr, out_dev, c->exec_stream, true);
  DPO_CHECK(hipEventRecord(c->done_event, c->exec_stream));
}

void dpo_eval_join(void* h, void* join_stream) {
  DpoCtx* c = (DpoCtx*)h;
  DPO_CHECK(hipStreamWaitEvent((hipStream_t)join_stream, c->done_event, 0));
}

}  // extern "C"

// --- batched agents: one launch per stage for a list of agents --------
// The agents of one colour are independent problems of the same shape
// (d, r), each of 2-6 workgroups per kernel. A batched wrapper (kb_*)
// serves a whole list with one launch: the last grid dimension is the
// agent, desc[agent] holds what the single-agent launch passes as
// arguments, and the wrapper calls the same *_body. A block at or beyond
// its own agent's extent returns at once, before any barrier, dot atomic
// or ticket, so every agent's block decomposition — and with it its
// arithmetic — is that of its single-agent launch. Guards are tested per
// agent on its own control block.
struct BatchDesc {
  // problem (DpoCtx::q_*, Minv) and G-assembly structure (DpoCtx::g_*)
  const int *q_rp, *q_ci;
  const double* q_vals;
  const float* Minv;
  const double* g_E0;
  const long *g_local_pose, *g_nbr_slot;
  const double* g_w;
  // iterate, packed neighbour buffer, linear term (nullptr: none)
  double* X;
  const double* nbr;
  const double* Gt;
  // work vectors and control block
  double *G_buf, *grad, *eta, *delta, *delta1, *rvec, *z, *Hd, *step, *Xprop;
  double *eta_snap, *delta_snap, *ctrl;
  double* prezero_z;  // ctx_prezero_z
  // TailArgs destinations and fences
  double* ctrl_host_dev;
  double* eval3;
  unsigned int* fences;
  long total, gtotal;  // gtotal: elements of G_buf to clear (0: no G term)
  int n, N, g_ne;
  // per-agent grid extents
  int nb_pose, nb_upd, nb_dense, jsplit, nb_gasm, nb_zero, nb_zero2, nb_copy;
};

static void batch_desc_extents(BatchDesc& b, int dh, int r) {
  b.nb_pose = blocks_for(b.n, 256);
  b.nb_upd = blocks_for((b.total + 3) / 4, 256);
  b.nb_dense = precond_dense_strips(b.N);
  b.jsplit = 1;  // the strip apply does not split j
  b.nb_gasm = blocks_for((long)b.g_ne * dh * r, 256);
  b.nb_zero = blocks_for(b.gtotal, 256);
  b.nb_zero2 = blocks_for(b.gtotal > CTRL_SIZE ? b.gtotal : (long)CTRL_SIZE,
                          256);
  b.nb_copy = blocks_for(b.total, 256);
}

__global__ void kb_dzero(const BatchDesc* __restrict__ desc) {
  const BatchDesc& a = desc[blockIdx.y];
  if ((int)blockIdx.x >= a.nb_zero) return;
  dzero_body(a.G_buf, a.gtotal);
}

__global__ void kb_dzero2(const BatchDesc* __restrict__ desc) {
  const BatchDesc& a = desc[blockIdx.y];
  if ((int)blockIdx.x >= a.nb_zero2) return;
  dzero2_body(a.G_buf, a.gtotal, a.ctrl, (long)CTRL_SIZE);
}

__global__ void kb_g_assemble(const BatchDesc* __restrict__ desc, int dh,
                              int r) {
  const BatchDesc& a = desc[blockIdx.y];
  if ((int)blockIdx.x >= a.nb_gasm) return;
  g_assemble_body(a.G_buf, a.g_E0, a.g_local_pose, a.g_nbr_slot, a.nbr,
                  a.g_w, a.g_ne, dh, r);
}

// The four Hessian stages of the dense chain, with the operands the
// per-agent sequence gives them (enqueue_solve_head, launch_hd_folded,
// enqueue_candidate, eval_terms).
enum BatchHess { BH_GRAD = 0, BH_HD = 1, BH_CAND = 2, BH_EVAL = 3 };

template <int D, int R, int ROLE, int CF>
__global__ void kb_hess(const BatchDesc* __restrict__ desc, TailArgs ta) {
  const BatchDesc& a = desc[blockIdx.y];
  if ((int)blockIdx.x >= a.nb_pose) return;
  const int s3 = a.Gt ? C_DOT2 : -1;
  if (ROLE == BH_GRAD) {
    hess_fused_body<D, R, 0, CF, 1>(a.q_rp, a.q_ci, a.q_vals, a.X, a.X, a.Gt,
                                    a.grad, nullptr, a.ctrl, a.n, C_DOT1,
                                    C_DOT0, s3, -1, a.rvec, a.prezero_z, ta,
                                    a.nb_pose);
  } else if (ROLE == BH_HD) {
    hess_fused_body<D, R, 0, CF, 2>(a.q_rp, a.q_ci, a.q_vals, nullptr, a.X,
                                    nullptr, a.Hd, a.z, a.ctrl, a.n, C_DOT0,
                                    -1, -1, ST_RUN, a.delta1, a.delta, ta,
                                    a.nb_pose);
  } else if (ROLE == BH_CAND) {
    ta.dst = a.ctrl_host_dev;
    ta.fence = a.fences + F_SOLVE_OUT;
    hess_fused_body<D, R, 1, CF, 0>(a.q_rp, a.q_ci, a.q_vals, a.Xprop,
                                    nullptr, a.Gt, nullptr, nullptr, a.ctrl,
                                    a.n, C_DOT0, C_DOT2, -1, ST_TCG_STOP,
                                    nullptr, nullptr, ta, a.nb_pose);
  } else {
    ta.dst = a.eval3;
    ta.fence = a.fences + F_EVAL_OUT;
    hess_fused_body<D, R, 0, CF, 0>(a.q_rp, a.q_ci, a.q_vals, a.X, a.X, a.Gt,
                                    a.grad, nullptr, a.ctrl, a.n, C_DOT1,
                                    C_DOT0, s3, -1, nullptr, nullptr, ta,
                                    a.nb_pose);
  }
}

// z = Minv rvec; grid (max strips, agents). VEC only when every agent of
// the batch is eligible (BatchExtents::vec); the bits do not depend on it.
template <int R, bool VEC>
__global__ void __launch_bounds__(256)
kb_precond_dense(const BatchDesc* __restrict__ desc) {
  const BatchDesc& a = desc[blockIdx.y];
  if ((int)blockIdx.x >= a.nb_dense) return;
  precond_dense_body<R, VEC>(a.Minv, a.rvec, a.z, a.N, a.ctrl, ST_RUN,
                             (int)blockIdx.x);
}

// z = P_X(z), <z, rvec>, tail CF_Z0 / CF_BETA
template <int D, int R, int CF>
__global__ void kb_proj_dots(const BatchDesc* __restrict__ desc) {
  const BatchDesc& a = desc[blockIdx.y];
  if ((int)blockIdx.x >= a.nb_pose) return;
  proj_dots_body<D, R, CF>(a.X, a.z, nullptr, a.z, a.rvec, a.ctrl, a.n,
                           C_DOT0, -1, ST_RUN, a.nb_pose);
}

template <int CF>
__global__ void kb_tcg_update(const BatchDesc* __restrict__ desc) {
  const BatchDesc& a = desc[blockIdx.y];
  if ((int)blockIdx.x >= a.nb_upd) return;
  tcg_update_body<CF>(a.eta, a.rvec, a.delta, a.Hd, a.eta_snap, a.delta_snap,
                      a.ctrl, a.total, a.prezero_z, a.delta1, a.nb_upd);
}

template <int D, int R>
__global__ void kb_candidate(const BatchDesc* __restrict__ desc) {
  const BatchDesc& a = desc[blockIdx.y];
  if ((int)blockIdx.x >= a.nb_pose) return;
  candidate_body<D, R>(a.ctrl, a.step, a.eta, a.eta_snap, a.delta_snap, a.X,
                       a.Xprop, a.n);
}

__global__ void kb_ctrl_tcg_end(const BatchDesc* __restrict__ desc) {
  ctrl_tcg_end_body(desc[blockIdx.y].ctrl);
}

// X <- Xprop for every agent whose bit is set in mask (the members that
// ended ST_ACCEPTED); replaces one device-to-device copy per agent.
__global__ void kb_commit(const BatchDesc* __restrict__ desc,
                          unsigned int mask) {
  if (!((mask >> blockIdx.y) & 1u)) return;
  const BatchDesc& a = desc[blockIdx.y];
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < a.total) a.X[i] = a.Xprop[i];
}

// Wait on and consume n fences, one lane per fence; the bounded spin of
// k_fence_wait.
__global__ void k_fence_wait_many(unsigned int* const* __restrict__ f,
                                  int n) {
  const int i = threadIdx.x;
  if (i < n) {
    long spins = 0;
    while (__hip_atomic_load(f[i], __ATOMIC_ACQUIRE,
                             __HIP_MEMORY_SCOPE_AGENT) == 0u) {
      __builtin_amdgcn_s_sleep(64);
      if (++spins > 30000000L) __builtin_trap();
    }
    __hip_atomic_store(f[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Grid extents of a batch: the maximum of every per-agent extent.
struct BatchExtents {
  int k = 0, pose = 1, upd = 1, dense = 1, gasm = 0, zero = 0, zero2 = 1,
      copy = 1;
  bool vec = true;  // every agent passes precond_dense_vec_ok
  void add(const BatchDesc& b) {
    ++k;
    pose = b.nb_pose > pose ? b.nb_pose : pose;
    upd = b.nb_upd > upd ? b.nb_upd : upd;
    dense = b.nb_dense > dense ? b.nb_dense : dense;
    vec = vec && precond_dense_vec_ok(b.Minv, b.N);
    gasm = b.nb_gasm > gasm ? b.nb_gasm : gasm;
    zero = b.nb_zero > zero ? b.nb_zero : zero;
    zero2 = b.nb_zero2 > zero2 ? b.nb_zero2 : zero2;
    copy = b.nb_copy > copy ? b.nb_copy : copy;
  }
};

// Launchers. d / r select the instantiation; dd is the device array.
template <int ROLE, int CF>
static void launch_kb_hess(const BatchDesc* dd, const BatchExtents& e, int d,
                           int r, const TailArgs& ta, hipStream_t s) {
  if (!dispatch_dr(d, r, [&](auto Dc, auto Rc) {
        hipLaunchKernelGGL((kb_hess<Dc, Rc, ROLE, CF>), dim3(e.pose, e.k),
                           dim3(256), 0, s, dd, ta);
      }))
    dpo_bad_shape(d, r);
}

static void launch_kb_precond(const BatchDesc* dd, const BatchExtents& e,
                              int r, hipStream_t s) {
  if (!dispatch_r(r, [&](auto Rc) {
        if (e.vec)
          hipLaunchKernelGGL((kb_precond_dense<Rc, true>),
                             dim3(e.dense, e.k), dim3(256), 0, s, dd);
        else
          hipLaunchKernelGGL((kb_precond_dense<Rc, false>),
                             dim3(e.dense, e.k), dim3(256), 0, s, dd);
      }))
    dpo_bad_shape(-1, r);
}

template <int CF>
static void launch_kb_proj(const BatchDesc* dd, const BatchExtents& e, int d,
                           int r, hipStream_t s) {
  if (!dispatch_dr(d, r, [&](auto Dc, auto Rc) {
        hipLaunchKernelGGL((kb_proj_dots<Dc, Rc, CF>), dim3(e.pose, e.k),
                           dim3(256), 0, s, dd);
      }))
    dpo_bad_shape(d, r);
}

static void launch_kb_candidate(const BatchDesc* dd, const BatchExtents& e,
                                int d, int r, hipStream_t s) {
  if (!dispatch_dr(d, r, [&](auto Dc, auto Rc) {
        hipLaunchKernelGGL((kb_candidate<Dc, Rc>), dim3(e.pose, e.k),
                           dim3(256), 0, s, dd);
      }))
    dpo_bad_shape(d, r);
}

static void launch_kb_gzero_assemble(const BatchDesc* dd,
                                     const BatchExtents& e, int d, int r,
                                     bool with_ctrl, hipStream_t s) {
  if (with_ctrl)
    hipLaunchKernelGGL(kb_dzero2, dim3(e.zero2, e.k), dim3(256), 0, s, dd);
  else if (e.zero > 0)
    hipLaunchKernelGGL(kb_dzero, dim3(e.zero, e.k), dim3(256), 0, s, dd);
  if (e.gasm > 0)
    hipLaunchKernelGGL(kb_g_assemble, dim3(e.gasm, e.k), dim3(256), 0, s, dd,
                       d + 1, r);
}

// The batched bodies: enqueue_solve_head / enqueue_tcg_iters /
// enqueue_solve_tail / enqueue_eval_body for the fused dense chain, one
// launch per stage. Linear, kernels only. fin: device array of the
// members' IN fences, consumed by the first node.
struct BatchShape { int d, r, max_inner; };

static void enqueue_batch_tcg_iters(const BatchDesc* dd,
                                    const BatchExtents& e,
                                    const BatchShape& sh, int count,
                                    hipStream_t s) {
  for (int j = 0; j < count; ++j) {
    launch_kb_hess<BH_HD, CF_ALPHA>(dd, e, sh.d, sh.r, TailArgs(), s);
    hipLaunchKernelGGL((kb_tcg_update<CF_RR>), dim3(e.upd, e.k), dim3(256),
                       0, s, dd);
    launch_kb_precond(dd, e, sh.r, s);
    launch_kb_proj<CF_BETA>(dd, e, sh.d, sh.r, s);
  }
}

static void enqueue_batch_tail(const BatchDesc* dd, const BatchExtents& e,
                               const BatchShape& sh, double accept_rho,
                               hipStream_t s) {
  launch_kb_candidate(dd, e, sh.d, sh.r, s);
  TailArgs ta;
  ta.a = accept_rho;
  // last node: every agent's last block publishes its control block and
  // releases its own F_SOLVE_OUT
  launch_kb_hess<BH_CAND, CF_ACCEPT_OUT>(dd, e, sh.d, sh.r, ta, s);
}

static void enqueue_batch_solve(const BatchDesc* dd, const BatchExtents& e,
                                const BatchShape& sh,
                                unsigned int* const* fin, double tol,
                                double Delta0, double accept_rho, int iters,
                                hipStream_t s) {
  hipLaunchKernelGGL(k_fence_wait_many, dim3(1), dim3(256), 0, s, fin, e.k);
  launch_kb_gzero_assemble(dd, e, sh.d, sh.r, /*with_ctrl=*/true, s);
  TailArgs ta;
  ta.a = tol; ta.b = Delta0; ta.c = 1.0; ta.d = 0.1;
  launch_kb_hess<BH_GRAD, CF_INIT>(dd, e, sh.d, sh.r, ta, s);
  launch_kb_precond(dd, e, sh.r, s);
  launch_kb_proj<CF_Z0>(dd, e, sh.d, sh.r, s);
  enqueue_batch_tcg_iters(dd, e, sh, iters, s);
  if (iters >= sh.max_inner)
    hipLaunchKernelGGL(kb_ctrl_tcg_end, dim3(1, e.k), dim3(64), 0, s, dd);
  enqueue_batch_tail(dd, e, sh, accept_rho, s);
}

static void enqueue_batch_cont(const BatchDesc* dd, const BatchExtents& e,
                               const BatchShape& sh,
                               unsigned int* const* fin, double accept_rho,
                               int done, hipStream_t s) {
  hipLaunchKernelGGL(k_fence_wait_many, dim3(1), dim3(256), 0, s, fin, e.k);
  enqueue_batch_tcg_iters(dd, e, sh, sh.max_inner - done, s);
  hipLaunchKernelGGL(kb_ctrl_tcg_end, dim3(1, e.k), dim3(64), 0, s, dd);
  enqueue_batch_tail(dd, e, sh, accept_rho, s);
}

static void enqueue_batch_eval(const BatchDesc* dd, const BatchExtents& e,
                               const BatchShape& sh,
                               unsigned int* const* fin, hipStream_t s) {
  hipLaunchKernelGGL(k_fence_wait_many, dim3(1), dim3(256), 0, s, fin, e.k);
  launch_kb_gzero_assemble(dd, e, sh.d, sh.r, /*with_ctrl=*/false, s);
  // every agent's last block writes its eval3 and releases F_EVAL_OUT
  launch_kb_hess<BH_EVAL, CF_EVAL>(dd, e, sh.d, sh.r, TailArgs(), s);
}

// DPO_BATCH=0 forces the per-agent path everywhere.
static bool batch_enabled() {
  static const bool on = [] {
    const char* v = getenv("DPO_BATCH");
    return !(v && v[0] == '0');
  }();
  return on;
}

// An agent can be a member of a batch: fused dense chain, thread-per-pose
// kernels, G assembled from a neighbour buffer.
static bool batch_ctx_ok(const DpoCtx* c, const double* nbr) {
  return c->Minv && ctx_fuse_scalar(c) && ctx_fold_delta(c) && nbr
         && c->q_rp;
}

static void batch_fill_desc(BatchDesc& b, DpoCtx* c, double* X,
                            const double* nbr) {
  memset(&b, 0, sizeof(b));
  b.q_rp = c->q_rp; b.q_ci = c->q_ci; b.q_vals = c->q_vals;
  b.Minv = c->Minv;
  b.g_E0 = c->g_E0; b.g_local_pose = c->g_local_pose;
  b.g_nbr_slot = c->g_nbr_slot; b.g_w = c->g_w; b.g_ne = c->g_ne;
  b.X = X; b.nbr = nbr;
  b.Gt = ctx_bind_round_g(c);
  b.G_buf = c->G_buf; b.grad = c->grad; b.eta = c->eta; b.delta = c->delta;
  b.delta1 = c->delta1; b.rvec = c->rvec; b.z = c->z; b.Hd = c->Hd;
  b.step = c->step; b.Xprop = c->Xprop; b.eta_snap = c->eta_snap;
  b.delta_snap = c->delta_snap; b.ctrl = c->ctrl;
  b.prezero_z = ctx_prezero_z(c);
  b.ctrl_host_dev = c->ctrl_host_dev; b.eval3 = c->eval3;
  b.fences = c->fences;
  b.total = c->total; b.gtotal = c->g_ne > 0 ? c->total : 0;
  b.n = c->n; b.N = c->N;
  batch_desc_extents(b, c->dh, c->r);
}

extern "C" {

// --- multi-agent round fan-out --------------------------------------
// The distributed driver runs one rank per GPU; within a rank several
// agents share the device. A round's per-agent enqueue loops (solve
// fan-out over the active color, eval fan-out over every agent) are
// pure launch overhead when driven from Python (~35 us/agent of
// interpreter + dispatcher time); DpoGroup runs each loop as ONE C
// call and gathers the per-agent eval scalars with a single kernel.

__global__ void k_gather3(double* __restrict__ out, long stride,
                          double* const* __restrict__ srcs,
                          const int* __restrict__ rows, int n) {
  int i = blockIdx.x;
  int j = threadIdx.x;
  if (i < n && j < 3) out[(long)rows[i] * stride + j] = srcs[i][j];
}

// Signal every agent's eval IN fence with one launch (lane per agent).
__global__ void k_fence_signal_many(unsigned int* const* __restrict__ f,
                                    int n) {
  int i = threadIdx.x;
  if (i < n)
    __hip_atomic_store(f[i], 1u, __ATOMIC_RELEASE,
                       __HIP_MEMORY_SCOPE_AGENT);
}

// Wait on & consume every agent's eval OUT fence, then gather each
// agent's 3 eval scalars (agent-scope loads: the producers ran on
// other XCDs) — replaces n (event-record + event-wait + copy) chains.
__global__ void k_gather3_fenced(double* __restrict__ out, long stride,
                                 double* const* __restrict__ srcs,
                                 const int* __restrict__ rows,
                                 unsigned int* const* __restrict__ f,
                                 int n) {
  int i = threadIdx.x;
  if (i < n) {
    long spins = 0;
    while (__hip_atomic_load(f[i], __ATOMIC_ACQUIRE,
                             __HIP_MEMORY_SCOPE_AGENT) == 0u) {
      __builtin_amdgcn_s_sleep(32);
      if (++spins > 30000000L) __builtin_trap();
    }
    __hip_atomic_store(f[i], 0u, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    #pragma unroll
    for (int j = 0; j < 3; ++j)
      out[(long)rows[i] * stride + j] = __hip_atomic_load(
          srcs[i] + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One cached batch: the agents of an active id list (or, for the
// evaluation, every agent of the group), their device descriptors and
// fence lists, and the graphs of the batched sequences.
#define BATCH_MAX_SOLVE 16  // members of a batched solve list
#define BATCH_MAX_LISTS 16  // cached active lists (colored: one per colour)
struct BatchSeq {
  int k = 0;
  int* ids = nullptr;
  long* stamps = nullptr;  // the members' desc_stamp at the last build
  bool built = false, ok = false;
  BatchDesc* d_desc = nullptr;
  unsigned int** d_fin = nullptr;   // members' IN fences
  unsigned int** d_fout = nullptr;  // members' OUT fences
  BatchExtents ext;
  BatchShape sh = {0, 0, 0};
  GraphCache primary, cont;
  void release() {
    primary.reset();
    cont.reset();
    dpo_ignore(hipFree(d_desc));
    dpo_ignore(hipFree(d_fin));
    dpo_ignore(hipFree(d_fout));
    free(ids);
    free(stamps);
  }
};

struct DpoGroup {
  int n;
  DpoCtx** cs;
  double** Xs;          // host arrays of fixed device pointers
  const double** nbrs;
  double** d_srcs;      // device array: each ctx's eval3
  int* d_rows;          // device array: output row per agent
  unsigned int** d_fin;   // device array: each ctx's F_EVAL_IN fence
  unsigned int** d_fout;  // device array: each ctx's F_EVAL_OUT fence
  // batched path: one execution and one capture stream for the group
  hipStream_t exec_stream = nullptr, cap_stream = nullptr;
  hipEvent_t done_event = nullptr;
  BatchSeq lists[BATCH_MAX_LISTS];
  int n_lists = 0;
  BatchSeq eval_seq;
  BatchSeq* pending = nullptr;  // batched solve in flight (start .. finish)
  double pend_rho = 0.0;
  // counters: batched solve rounds, batched continuations, batched
  // evaluations, per-agent solve rounds, per-agent evaluations, graph
  // captures, descriptor builds
  long n_bsolve = 0, n_bcont = 0, n_beval = 0, n_psolve = 0, n_peval = 0,
       n_capture = 0, n_build = 0;
};

// (Re)build a batch when it is new or a member's descriptor stamp moved:
// eligibility, descriptors, fence lists, extents; graphs are dropped
// when the extents changed.
// Returns whether the batch is eligible. eval selects the fence pair.
static bool batch_seq_refresh(DpoGroup* gr, BatchSeq& q, bool eval) {
  bool same = q.built;
  for (int i = 0; same && i < q.k; ++i)
    same = q.stamps[i] == gr->cs[q.ids[i]]->desc_stamp;
  if (same) return q.ok;
  // the old descriptors may still be in use by work on the group stream
  DPO_CHECK(hipStreamSynchronize(gr->exec_stream));
  const bool was_ok = q.built && q.ok;
  const BatchExtents old_ext = q.ext;
  const BatchShape old_sh = q.sh;
  q.built = true;
  q.ok = q.k >= 2;
  const DpoCtx* c0 = gr->cs[q.ids[0]];
  for (int i = 0; i < q.k; ++i) {
    const DpoCtx* c = gr->cs[q.ids[i]];
    q.stamps[i] = c->desc_stamp;
    q.ok = q.ok && batch_ctx_ok(c, gr->nbrs[q.ids[i]]) && c->d == c0->d
           && c->r == c0->r && c->max_inner == c0->max_inner;
  }
  if (!q.ok) {
    q.primary.reset();
    q.cont.reset();
    return false;
  }
  gr->n_build++;
  q.sh = {c0->d, c0->r, c0->max_inner};
  BatchDesc* hd = (BatchDesc*)malloc(q.k * sizeof(BatchDesc));
  unsigned int** hin = (unsigned int**)malloc(q.k * sizeof(void*));
  unsigned int** hout = (unsigned int**)malloc(q.k * sizeof(void*));
  q.ext = BatchExtents();
  for (int i = 0; i < q.k; ++i) {
    DpoCtx* c = gr->cs[q.ids[i]];
    batch_fill_desc(hd[i], c, gr->Xs[q.ids[i]], gr->nbrs[q.ids[i]]);
    q.ext.add(hd[i]);
    hin[i] = c->fences + (eval ? F_EVAL_IN : F_SOLVE_IN);
    hout[i] = c->fences + (eval ? F_EVAL_OUT : F_SOLVE_OUT);
  }
  if (!q.d_desc) {
    DPO_CHECK(hipMalloc(&q.d_desc, q.k * sizeof(BatchDesc)));
    DPO_CHECK(hipMalloc(&q.d_fin, q.k * sizeof(void*)));
    DPO_CHECK(hipMalloc(&q.d_fout, q.k * sizeof(void*)));
  }
  DPO_CHECK(hipMemcpy(q.d_desc, hd, q.k * sizeof(BatchDesc),
                      hipMemcpyHostToDevice));
  DPO_CHECK(hipMemcpy(q.d_fin, hin, q.k * sizeof(void*),
                      hipMemcpyHostToDevice));
  DPO_CHECK(hipMemcpy(q.d_fout, hout, q.k * sizeof(void*),
                      hipMemcpyHostToDevice));
  free(hd); free(hin); free(hout);
  // The graphs' kernels take the descriptor array (same allocation) and
  // scalars as arguments, and their grids come from the extents: a member
  // whose buffers moved but whose sizes did not (a preconditioner refresh
  // allocates a new Minv) needs new descriptors, not a recapture.
  if (!was_ok || memcmp(&old_ext, &q.ext, sizeof(old_ext)) != 0
      || memcmp(&old_sh, &q.sh, sizeof(old_sh)) != 0) {
    q.primary.reset();
    q.cont.reset();
  }
  return true;
}

static void batch_seq_init(BatchSeq& q, const int* ids, int k) {
  q.k = k;
  q.ids = (int*)malloc(k * sizeof(int));
  q.stamps = (long*)malloc(k * sizeof(long));
  for (int i = 0; i < k; ++i) q.ids[i] = ids ? ids[i] : i;
}

// The cached batch of an active list; nullptr when the list cannot be
// batched (the caller then takes the per-agent path).
static BatchSeq* group_solve_batch(DpoGroup* gr, const int* ids, int k) {
  static const bool no_graph = dpo_env_flag("DPO_NO_SOLVE_GRAPH");
  if (!batch_enabled() || no_graph || k < 2 || k > BATCH_MAX_SOLVE)
    return nullptr;
  BatchSeq* q = nullptr;
  for (int l = 0; l < gr->n_lists && !q; ++l)
    if (gr->lists[l].k == k
        && memcmp(gr->lists[l].ids, ids, k * sizeof(int)) == 0)
      q = &gr->lists[l];
  if (!q) {
    if (gr->n_lists >= BATCH_MAX_LISTS) return nullptr;
    for (int i = 0; i < k; ++i)
      if (ids[i] < 0 || ids[i] >= gr->n) return nullptr;
    q = &gr->lists[gr->n_lists++];
    batch_seq_init(*q, ids, k);
  }
  return batch_seq_refresh(gr, *q, /*eval=*/false) ? q : nullptr;
}

void dpo_group_destroy(void* g) {
  DpoGroup* gr = (DpoGroup*)g;
  if (!gr) return;
  if (gr->exec_stream) dpo_ignore(hipStreamSynchronize(gr->exec_stream));
  for (int l = 0; l < gr->n_lists; ++l) gr->lists[l].release();
  gr->eval_seq.release();
  if (gr->exec_stream) dpo_ignore(hipStreamDestroy(gr->exec_stream));
  if (gr->cap_stream) dpo_ignore(hipStreamDestroy(gr->cap_stream));
  if (gr->done_event) dpo_ignore(hipEventDestroy(gr->done_event));
  dpo_ignore(hipFree(gr->d_srcs));
  dpo_ignore(hipFree(gr->d_rows));
  dpo_ignore(hipFree(gr->d_fin));
  dpo_ignore(hipFree(gr->d_fout));
  free(gr->cs); free(gr->Xs); free(gr->nbrs);
  delete gr;
}

void* dpo_group_create(void** handles, int n, double** Xs,
                       const double** nbrs, const int* rows) {
  if (n <= 0 || n > 256) return nullptr;
  DpoGroup* gr = new DpoGroup();
  gr->n = n;
  gr->cs = (DpoCtx**)malloc(n * sizeof(void*));
  gr->Xs = (double**)malloc(n * sizeof(void*));
  gr->nbrs = (const double**)malloc(n * sizeof(void*));
  double* srcs_h[256];
  unsigned int* fin_h[256];
  unsigned int* fout_h[256];
  for (int i = 0; i < n; ++i) {
    gr->cs[i] = (DpoCtx*)handles[i];
    gr->Xs[i] = Xs[i];
    gr->nbrs[i] = nbrs[i];
    srcs_h[i] = gr->cs[i]->eval3;
    fin_h[i] = gr->cs[i]->fences + F_EVAL_IN;
    fout_h[i] = gr->cs[i]->fences + F_EVAL_OUT;
  }
  DPO_CHECK(hipMalloc(&gr->d_srcs, n * sizeof(double*)));
  DPO_CHECK(hipMemcpy(gr->d_srcs, srcs_h, n * sizeof(double*),
                      hipMemcpyHostToDevice));
  DPO_CHECK(hipMalloc(&gr->d_rows, n * sizeof(int)));
  DPO_CHECK(hipMemcpy(gr->d_rows, rows, n * sizeof(int),
                      hipMemcpyHostToDevice));
  DPO_CHECK(hipMalloc(&gr->d_fin, n * sizeof(void*)));
  DPO_CHECK(hipMemcpy(gr->d_fin, fin_h, n * sizeof(void*),
                      hipMemcpyHostToDevice));
  DPO_CHECK(hipMalloc(&gr->d_fout, n * sizeof(void*)));
  DPO_CHECK(hipMemcpy(gr->d_fout, fout_h, n * sizeof(void*),
                      hipMemcpyHostToDevice));
  DPO_CHECK(hipStreamCreateWithFlags(&gr->exec_stream,
                                     hipStreamNonBlocking));
  DPO_CHECK(hipStreamCreateWithFlags(&gr->cap_stream, hipStreamNonBlocking));
  DPO_CHECK(hipEventCreateWithFlags(&gr->done_event,
                                    hipEventDisableTiming));
  batch_seq_init(gr->eval_seq, nullptr, n);
  return gr;
}

// Solves of the active agents (indices into the group).
//
// Batched (an eligible list, see group_solve_batch): one signal launch on
// the join stream, one graph launch and one wait launch on the group's
// stream. Otherwise the fan-out over each agent's private exec stream.
//
// The two paths may alternate from round to round. Ordering between them
// always passes through the join stream: every IN fence is signalled
// there, behind whatever the join stream has waited for, and every path
// ends by making the join stream wait for its done event (solves) or its
// OUT fences (evaluation). Neither path relies on the order of two
// execution streams against each other.
void dpo_group_solve_start(void* g, const int* ids, int k, double tol,
                           double Delta0, double accept_rho,
                           void* join_stream) {
  DpoGroup* gr = (DpoGroup*)g;
  hipStream_t js = (hipStream_t)join_stream;
  BatchSeq* q = group_solve_batch(gr, ids, k);
  gr->pending = q;
  if (!q) {
    gr->n_psolve++;
    for (int i = 0; i < k; ++i) {
      int a = ids[i];
      dpo_round_solve_async(gr->cs[a], gr->Xs[a], gr->nbrs[a], tol, Delta0,
                            accept_rho, join_stream);
    }
    return;
  }
  gr->n_bsolve++;
  gr->pend_rho = accept_rho;
  for (int i = 0; i < k; ++i) ctx_bind_round_g(gr->cs[ids[i]]);
  hipStream_t s = gr->exec_stream;
  hipLaunchKernelGGL(k_fence_signal_many, dim3(1), dim3(256), 0, js,
                     (unsigned int* const*)q->d_fin, q->k);
  const int seg = solve_segment(gr->cs[ids[0]]);
  const void* key[4] = {q->d_desc, (const void*)(intptr_t)(tol * 1e9),
                        (const void*)(intptr_t)Delta0,
                        (const void*)(intptr_t)(accept_rho * 1e9)};
  const bool launched = graph_cache_launch(
      q->primary, key, gr->cap_stream, s, [&](hipStream_t cs) {
        gr->n_capture++;
        enqueue_batch_solve(q->d_desc, q->ext, q->sh, q->d_fin, tol, Delta0,
                            accept_rho, seg, cs);
      });
  if (!launched)  // capture unavailable: the whole sequence, eagerly
    enqueue_batch_solve(q->d_desc, q->ext, q->sh, q->d_fin, tol, Delta0,
                        accept_rho, q->sh.max_inner, s);
  hipLaunchKernelGGL(k_fence_wait_many, dim3(1), dim3(256), 0, s,
                     (unsigned int* const*)q->d_fout, q->k);
}

void dpo_group_solve_finish(void* g, const int* ids, int k,
                            int max_shrink, void* join_stream) {
  DpoGroup* gr = (DpoGroup*)g;
  hipStream_t js = (hipStream_t)join_stream;
  BatchSeq* q = gr->pending;
  gr->pending = nullptr;
  if (q) {
    hipStream_t s = gr->exec_stream;
    DPO_CHECK(hipStreamSynchronize(s));
    // members still running get the rest of their iterations from the
    // batched continuation. It runs for the whole list: the finished
    // members' guarded kernels are no-ops, their unguarded publish step
    // republishes and re-releases, so IN and OUT fences are handled the
    // same for every member. (A member whose first candidate was rejected
    // re-evaluates that same candidate; it then shrinks as usual.)
    const int seg = solve_segment(gr->cs[ids[0]]);
    bool any_run = false;
    if (seg < q->sh.max_inner)
      for (int i = 0; i < k; ++i) {
        DpoCtx* c = gr->cs[ids[i]];
        if ((int)c->ctrl_host[C_STATUS] == ST_RUN) {
          c->n_conts++;
          any_run = true;
        }
      }
    if (any_run) {
      gr->n_bcont++;
      hipLaunchKernelGGL(k_fence_signal_many, dim3(1), dim3(256), 0, s,
                         (unsigned int* const*)q->d_fin, q->k);
      const void* key[4] = {q->d_desc, nullptr, nullptr,
                            (const void*)(intptr_t)(gr->pend_rho * 1e9)};
      const bool launched = graph_cache_launch(
          q->cont, key, gr->cap_stream, s, [&](hipStream_t cs) {
            gr->n_capture++;
            enqueue_batch_cont(q->d_desc, q->ext, q->sh, q->d_fin,
                               gr->pend_rho, seg, cs);
          });
      if (!launched)
        enqueue_batch_cont(q->d_desc, q->ext, q->sh, q->d_fin, gr->pend_rho,
                           seg, s);
      hipLaunchKernelGGL(k_fence_wait_many, dim3(1), dim3(256), 0, s,
                         (unsigned int* const*)q->d_fout, q->k);
      DPO_CHECK(hipStreamSynchronize(s));
    }
    // acceptance, the (rare) shrink loop and the counters per agent, on
    // the group's stream; then one launch commits X <- Xprop for every
    // member that ended accepted
    unsigned int mask = 0;
    for (int i = 0; i < k; ++i) {
      DpoCtx* c = gr->cs[ids[i]];
      const int st = solve_postsync(c, gr->Xs[ids[i]], gr->pend_rho,
                                    max_shrink, 0, nullptr, s,
                                    /*commit=*/false);
      if (st == ST_ACCEPTED) mask |= 1u << i;
    }
    if (mask)
      hipLaunchKernelGGL(kb_commit, dim3(q->ext.copy, q->k), dim3(256), 0, s,
                         q->d_desc, mask);
    DPO_CHECK(hipEventRecord(gr->done_event, s));
    DPO_CHECK(hipStreamWaitEvent(js, gr->done_event, 0));
    return;
  }
  bool continued[256];  // dpo_group_create caps a group at 256 agents
  // pass 1: an agent that needs no continuation is finished at once, as
  // before; one that does only gets its continuation launched
  for (int i = 0; i < k && i < 256; ++i) {
    continued[i] = round_finish_primary(gr->cs[ids[i]]);
    if (!continued[i])
      round_finish_post(gr->cs[ids[i]], false, max_shrink, nullptr, js);
  }
  // pass 2: the continued agents
  for (int i = 0; i < k && i < 256; ++i)
    if (continued[i])
      round_finish_post(gr->cs[ids[i]], true, max_shrink, nullptr, js);
}

// Evaluation of EVERY agent in the group into its eval3 scratch, then
// all rows gathered into out_dev[rows[i]*row_stride .. +3] with one
// kernel on join_stream. Batched (every agent eligible): one signal
// launch, one graph launch on the group's stream, the gather. Otherwise
// the fan-out over the per-agent exec streams.
void dpo_group_eval(void* g, double* out_dev, long row_stride,
                    void* join_stream) {
  DpoGroup* gr = (DpoGroup*)g;
  hipStream_t js = (hipStream_t)join_stream;
  static const bool no_graph = dpo_env_flag("DPO_NO_EVAL_GRAPH");
  const bool batched = batch_enabled() && !no_graph
                       && batch_seq_refresh(gr, gr->eval_seq, /*eval=*/true);
  // one kernel signals every agent's IN fence (carries the boundary
  // scatter ordering); the evaluation graphs are then launched bare on
  // their exec streams — no event ceremony — and one gather kernel on the
  // join stream waits on & consumes every OUT fence.
  hipLaunchKernelGGL(k_fence_signal_many, dim3(1), dim3(256), 0, js,
                     (unsigned int* const*)gr->d_fin, gr->n);
  if (batched) {
    BatchSeq& q = gr->eval_seq;
    gr->n_beval++;
    for (int i = 0; i < gr->n; ++i) ctx_bind_round_g(gr->cs[i]);
    const void* key[4] = {q.d_desc, nullptr, nullptr, nullptr};
    const bool launched = graph_cache_launch(
        q.primary, key, gr->cap_stream, gr->exec_stream,
        [&](hipStream_t cs) {
          gr->n_capture++;
          enqueue_batch_eval(q.d_desc, q.ext, q.sh, q.d_fin, cs);
        });
    if (!launched)
      enqueue_batch_eval(q.d_desc, q.ext, q.sh, q.d_fin, gr->exec_stream);
  } else {
    gr->n_peval++;
    for (int i = 0; i < gr->n; ++i)
      round_eval_impl(gr->cs[i], gr->Xs[i], gr->nbrs[i], gr->cs[i]->eval3,
                      gr->cs[i]->exec_stream, /*wait_out=*/false);
  }
  hipLaunchKernelGGL(k_gather3_fenced, dim3(1), dim3(256), 0, js,
                     out_dev, row_stride, gr->d_srcs, gr->d_rows,
                     (unsigned int* const*)gr->d_fout, gr->n);
}

// out[0..6] = batched solve rounds, batched continuations, batched
// evaluations, per-agent solve rounds, per-agent evaluations, graph
// captures of the batched sequences, descriptor builds. Writes at most
// `cap` entries; returns the full length.
int dpo_group_counters(void* g, long* out, int cap) {
  DpoGroup* gr = (DpoGroup*)g;
  const long v[7] = {gr->n_bsolve, gr->n_bcont, gr->n_beval, gr->n_psolve,
                     gr->n_peval, gr->n_capture, gr->n_build};
  for (int i = 0; i < 7 && i < cap; ++i) out[i] = v[i];
  return 7;
}

// --- the batched wrappers as stand-alone ops (tests) -----------------
// Test support, like dpo_hd_stage / dpo_candidate / dpo_hess_tail above:
// nothing in the package calls these two.
int dpo_batch_desc_size() { return (int)sizeof(BatchDesc); }

// One batched wrapper on caller-owned descriptors (tests): descs_host is
// an array of k BatchDesc whose pointer fields are set; the extents are
// filled in here. Uploads, launches on `stream` and synchronises.
//   0 kb_dzero          1 kb_dzero2        2 kb_g_assemble
//   3 gradient + CF_INIT (a = tol, b = Delta0)
//   4 folded Hd + CF_ALPHA
//   5 candidate evaluation + CF_ACCEPT_OUT (a = accept_rho)
//   6 candidate evaluation + CF_ACCEPT     (a = accept_rho)
//   7 evaluation + CF_EVAL
//   8 kb_precond_dense  9 kb_proj_dots CF_Z0   10 kb_proj_dots CF_BETA
//  11 kb_tcg_update CF_RR   12 kb_candidate    13 kb_ctrl_tcg_end
//  14 kb_commit (mask = (unsigned)a)
int dpo_batch_op(int op, void* descs_host, int k, int d, int r, double a,
                 double b, void* stream) {
  if (k <= 0 || k > 32) return -1;
  hipStream_t s = (hipStream_t)stream;
  BatchDesc* hd = (BatchDesc*)descs_host;
  BatchExtents e;
  for (int i = 0; i < k; ++i) {
    batch_desc_extents(hd[i], d + 1, r);
    e.add(hd[i]);
  }
  BatchDesc* dd = nullptr;
  DPO_CHECK(hipMalloc(&dd, k * sizeof(BatchDesc)));
  DPO_CHECK(hipMemcpy(dd, hd, k * sizeof(BatchDesc), hipMemcpyHostToDevice));
  TailArgs ta;
  ta.a = a; ta.b = b; ta.c = 1.0; ta.d = 0.1;
  int rc = 0;
  switch (op) {
    case 0:
      if (e.zero > 0)
        hipLaunchKernelGGL(kb_dzero, dim3(e.zero, k), dim3(256), 0, s, dd);
      break;
    case 1:
      hipLaunchKernelGGL(kb_dzero2, dim3(e.zero2, k), dim3(256), 0, s, dd);
      break;
    case 2:
      if (e.gasm > 0)
        hipLaunchKernelGGL(kb_g_assemble, dim3(e.gasm, k), dim3(256), 0, s,
                           dd, d + 1, r);
      break;
    case 3: launch_kb_hess<BH_GRAD, CF_INIT>(dd, e, d, r, ta, s); break;
    case 4: launch_kb_hess<BH_HD, CF_ALPHA>(dd, e, d, r, ta, s); break;
    case 5: launch_kb_hess<BH_CAND, CF_ACCEPT_OUT>(dd, e, d, r, ta, s); break;
    case 6: launch_kb_hess<BH_CAND, CF_ACCEPT>(dd, e, d, r, ta, s); break;
    case 7: launch_kb_hess<BH_EVAL, CF_EVAL>(dd, e, d, r, ta, s); break;
    case 8: launch_kb_precond(dd, e, r, s); break;
    case 9: launch_kb_proj<CF_Z0>(dd, e, d, r, s); break;
    case 10: launch_kb_proj<CF_BETA>(dd, e, d, r, s); break;
    case 11:
      hipLaunchKernelGGL((kb_tcg_update<CF_RR>), dim3(e.upd, k), dim3(256),
                         0, s, dd);
      break;
    case 12: launch_kb_candidate(dd, e, d, r, s); break;
    case 13:
      hipLaunchKernelGGL(kb_ctrl_tcg_end, dim3(1, k), dim3(64), 0, s, dd);
      break;
    case 14:
      hipLaunchKernelGGL(kb_commit, dim3(e.copy, k), dim3(256), 0, s, dd,
                         (unsigned int)a);
      break;
    default: rc = -1; break;
  }
  DPO_CHECK(hipStreamSynchronize(s));
  dpo_ignore(hipFree(dd));
  return rc;
}

}  // extern "C"

// =====================================================================
// Optimality certificate: S = Q - Lambda(X) and Lanczos with full
// reorthogonalisation (docs/DESIGN.md §14). Purely additive: none of the
// solve/eval kernels above is used or changed, except that Q @ X comes
// from k_bsr_spmm.
//
// Reductions are run-to-run deterministic: every block
// reduces in a fixed shuffle/LDS order and stores ONE partial into a
// per-block slot; the consuming kernel (always a later launch, so the
// kernel boundary publishes the slots) sums the <= CERT_MAX_PART
// partials in the same fixed order. No floating-point atomics.
//
// Control array `cc` (fp64): flag, completed-step count, breakdown
// threshold, then alpha[m] and beta[m]. Once the flag is set every
// later kernel of the enqueued batch returns at once (the guard idiom
// of the solve kernels), so no step divides by a vanished beta.
// =====================================================================
enum CertSlot {
  CC_FLAG = 0,   // != 0: Krylov space exhausted (breakdown)
  CC_COUNT = 1,  // completed Lanczos steps (alpha_j, beta_j valid)
  CC_TOL = 2,    // absolute breakdown threshold on beta
  CC_HDR = 4,    // alpha[j] at CC_HDR + j, beta[j] at CC_HDR + m + j
};
#define CERT_MAX_PART 256
#define CERT_BS 256

static inline int cert_grid(long total) {
  const int g = blocks_for(total, CERT_BS);
  return g < CERT_MAX_PART ? g : CERT_MAX_PART;
}

__device__ __forceinline__ bool cert_off(const double* cc) {
  return cc != nullptr && cc[CC_FLAG] != 0.0;
}

// Fixed-order block sum (blockDim.x == CERT_BS); every thread returns
// the same value.
__device__ __forceinline__ double cert_block_sum(double v) {
  __shared__ double sh[CERT_BS / 64];
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = sh[0];
  #pragma unroll
  for (int w = 1; w < CERT_BS / 64; ++w) s += sh[w];
  __syncthreads();  // sh is reused by the next reduction in this kernel
  return s;
}

__device__ __forceinline__ double cert_sum_partials(const double* part,
                                                    int npart) {
  const int t = threadIdx.x;
  return cert_block_sum(t < npart ? part[t] : 0.0);
}

// out[0] = sum of the per-block partials (single block)
__global__ void k_cert_reduce(const double* __restrict__ part, int npart,
                              double* __restrict__ out) {
  const double s = cert_sum_partials(part, npart);
  if (threadIdx.x == 0) out[0] = s;
}

// Lambda blocks and the criticality residual. One thread per pose:
//   Lambda_i = sym(QX_i X_i^T) on the d rotation rows (d x d),
//   part[b]  = block partial of ||QX - Lambda X||_F^2 (the translation
//              row of Lambda is zero, so its rows contribute QX^2).
template <int D, int R>
__global__ void k_cert_lambda(const double* __restrict__ X,
                              const double* __restrict__ QX,
                              double* __restrict__ lam,
                              double* __restrict__ part, int n) {
  constexpr int dh = D + 1;
  double res = 0.0;
  for (int i = blockIdx.x * CERT_BS + threadIdx.x; i < n;
       i += gridDim.x * CERT_BS) {
    const double* Xi = X + (size_t)i * dh * R;
    const double* Gi = QX + (size_t)i * dh * R;
    double Y[D][R], G[D][R];
    #pragma unroll
    for (int a = 0; a < D; ++a)
      #pragma unroll
      for (int k = 0; k < R; ++k) {
        Y[a][k] = Xi[a * R + k];
        G[a][k] = Gi[a * R + k];
      }
    double L[D][D];
    #pragma unroll
    for (int a = 0; a < D; ++a)
      #pragma unroll
      for (int b = a; b < D; ++b) {
        double s = 0.0;
        #pragma unroll
        for (int k = 0; k < R; ++k)
          s = fma(G[a][k], Y[b][k], fma(G[b][k], Y[a][k], s));
        s *= 0.5;
        L[a][b] = s;
        L[b][a] = s;
      }
    #pragma unroll
    for (int a = 0; a < D; ++a)
      #pragma unroll
      for (int b = 0; b < D; ++b)
        lam[(size_t)i * D * D + a * D + b] = L[a][b];
    #pragma unroll
    for (int a = 0; a < D; ++a)
      #pragma unroll
      for (int k = 0; k < R; ++k) {
        double g = G[a][k];
        #pragma unroll
        for (int b = 0; b < D; ++b) g = fma(-L[a][b], Y[b][k], g);
        res = fma(g, g, res);
      }
    #pragma unroll
    for (int k = 0; k < R; ++k) {
      const double g = Gi[D * R + k];
      res = fma(g, g, res);
    }
  }
  const double s = cert_block_sum(res);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// One fused Lanczos step on a single vector, one thread per scalar row
// (BSR traversal of k_bsr_spmm with r = 1):
//   w_i = sum_j Q_ij v_j - Lambda_i v_i - beta_prev * vprev_i
//   part[b] = block partial of alpha = <v, w>
// beta_prev is read from a device slot (nullptr: first step, 0).
template <int D>
__global__ void k_cert_apply(const int* __restrict__ row_ptr,
                             const int* __restrict__ col_idx,
                             const double* __restrict__ vals,
                             const double* __restrict__ lam,
                             const double* __restrict__ v,
                             const double* __restrict__ vprev,
                             const double* __restrict__ beta_prev,
                             double* __restrict__ w,
                             double* __restrict__ part, int n,
                             const double* __restrict__ cc) {
  if (cert_off(cc)) return;
  constexpr int DH = D + 1;
  const long N = (long)n * DH;
  const double beta = (beta_prev && vprev) ? beta_prev[0] : 0.0;
  double dot = 0.0;
  for (long row = (long)blockIdx.x * CERT_BS + threadIdx.x; row < N;
       row += (long)gridDim.x * CERT_BS) {
    const int i = (int)(row / DH);
    const int c = (int)(row % DH);
    const int s = row_ptr[i], e = row_ptr[i + 1];
    double acc = 0.0;
    for (int p = s; p < e; ++p) {
      const double* B = vals + (size_t)p * DH * DH + c * DH;
      const double* vj = v + (size_t)col_idx[p] * DH;
      #pragma unroll
      for (int cc2 = 0; cc2 < DH; ++cc2) acc = fma(B[cc2], vj[cc2], acc);
    }
    if (c < D) {
      const double* Li = lam + (size_t)i * D * D + c * D;
      const double* vi = v + (size_t)i * DH;
      #pragma unroll
      for (int b = 0; b < D; ++b) acc = fma(-Li[b], vi[b], acc);
    }
    if (vprev) acc = fma(-beta, vprev[row], acc);
    w[row] = acc;
    dot = fma(v[row], acc, dot);
  }
  const double sdot = cert_block_sum(dot);
  if (threadIdx.x == 0) part[blockIdx.x] = sdot;
}

// c = V^T w against the stored basis (column-major, ncols columns of
// length N): one workgroup per basis column. Block 0 of the first pass
// also finalises alpha from k_cert_apply's partials.
__global__ void k_cert_gram(const double* __restrict__ V,
                            const double* __restrict__ w,
                            double* __restrict__ c, long N,
                            const double* __restrict__ cc,
                            const double* __restrict__ part, int npart,
                            double* __restrict__ alpha_out) {
  if (cert_off(cc)) return;
  const double* Vk = V + (size_t)blockIdx.x * N;
  double dot = 0.0;
  for (long row = threadIdx.x; row < N; row += CERT_BS)
    dot = fma(Vk[row], w[row], dot);
  const double s = cert_block_sum(dot);
  if (threadIdx.x == 0) c[blockIdx.x] = s;
  if (alpha_out != nullptr && blockIdx.x == 0) {
    const double a = cert_sum_partials(part, npart);
    if (threadIdx.x == 0) alpha_out[0] = a;
  }
}

// Row-split c = V^T w for the restarted path: the rows of N are divided
// over the grid, each block handles its rows for all ncols columns in
// tiles of CERT_GRAM_CT columns (w is re-read once per tile, 1/CT of the
// V traffic) and stores one partial per (column, block) at
// gpart[col * gridDim.x + block]. A tail tile clamps the column index
// and discards the duplicate sums. k_cert_gram_finish sums the slots.
#define CERT_GRAM_CT 8
__global__ void k_cert_gram_split(const double* __restrict__ V,
                                  const double* __restrict__ w,
                                  double* __restrict__ gpart, int ncols,
                                  long N, const double* __restrict__ cc) {
  if (cert_off(cc)) return;
  for (int c0 = 0; c0 < ncols; c0 += CERT_GRAM_CT) {
    const double* Vc[CERT_GRAM_CT];
    #pragma unroll
    for (int c = 0; c < CERT_GRAM_CT; ++c) {
      const int col = c0 + c < ncols ? c0 + c : ncols - 1;
      Vc[c] = V + (size_t)col * N;
    }
    double acc[CERT_GRAM_CT];
    #pragma unroll
    for (int c = 0; c < CERT_GRAM_CT; ++c) acc[c] = 0.0;
    for (long row = (long)blockIdx.x * CERT_BS + threadIdx.x; row < N;
         row += (long)gridDim.x * CERT_BS) {
      const double wr = w[row];
      #pragma unroll
      for (int c = 0; c < CERT_GRAM_CT; ++c)
        acc[c] = fma(Vc[c][row], wr, acc[c]);
    }
    #pragma unroll
    for (int c = 0; c < CERT_GRAM_CT; ++c) {
      const double s = cert_block_sum(acc[c]);
      if (threadIdx.x == 0 && c0 + c < ncols)
        gpart[(size_t)(c0 + c) * gridDim.x + blockIdx.x] = s;
    }
  }
}

// c[col] = fixed-order sum of column col's ngrid row-split partials, one
// workgroup per column; block 0 of the first pass also finalises alpha
// from k_cert_apply's partials, as k_cert_gram does.
__global__ void k_cert_gram_finish(const double* __restrict__ gpart,
                                   int ngrid, double* __restrict__ c,
                                   const double* __restrict__ cc,
                                   const double* __restrict__ part,
                                   int npart,
                                   double* __restrict__ alpha_out) {
  if (cert_off(cc)) return;
  const double s =
      cert_sum_partials(gpart + (size_t)blockIdx.x * ngrid, ngrid);
  if (threadIdx.x == 0) c[blockIdx.x] = s;
  if (alpha_out != nullptr && blockIdx.x == 0) {
    const double a = cert_sum_partials(part, npart);
    if (threadIdx.x == 0) alpha_out[0] = a;
  }
}

// Thick-restart basis contraction, in place: V[0..k) <- C^T V[0..b),
// V[k] <- V[b]. V is b + 1 contiguous vectors of length N; C is b rows of
// CERT_KEEP_MAX coefficients (columns >= k are zero padding). One thread
// owns row index i: it reads V[0..b][i] (coalesced across the wave) into
// CERT_KEEP_MAX register accumulators and stores only after its last
// load, and no other thread touches index i, so in place is safe. V is
// deliberately not __restrict__: the stores alias the loads.
#define CERT_KEEP_MAX 16
__global__ void k_cert_contract(double* V, const double* __restrict__ C,
                                int b, int k, long N) {
  for (long i = (long)blockIdx.x * CERT_BS + threadIdx.x; i < N;
       i += (long)gridDim.x * CERT_BS) {
    double acc[CERT_KEEP_MAX];
    #pragma unroll
    for (int c = 0; c < CERT_KEEP_MAX; ++c) acc[c] = 0.0;
    for (int j = 0; j < b; ++j) {
      const double x = V[(size_t)j * N + i];
      #pragma unroll
      for (int c = 0; c < CERT_KEEP_MAX; ++c)
        acc[c] = fma(C[j * CERT_KEEP_MAX + c], x, acc[c]);
    }
    const double carry = V[(size_t)b * N + i];
    #pragma unroll
    for (int c = 0; c < CERT_KEEP_MAX; ++c)
      if (c < k) V[(size_t)c * N + i] = acc[c];
    V[(size_t)k * N + i] = carry;
  }
}

// w -= V c; with part != nullptr also the block partials of ||w||^2.
__global__ void k_cert_sub(const double* __restrict__ V,
                           const double* __restrict__ c,
                           double* __restrict__ w, int ncols, long N,
                           const double* __restrict__ cc,
                           double* __restrict__ part) {
  if (cert_off(cc)) return;
  double nrm = 0.0;
  for (long row = (long)blockIdx.x * CERT_BS + threadIdx.x; row < N;
       row += (long)gridDim.x * CERT_BS) {
    double acc = w[row];
    for (int k = 0; k < ncols; ++k)
      acc = fma(-c[k], V[(size_t)k * N + row], acc);
    w[row] = acc;
    nrm = fma(acc, acc, nrm);
  }
  if (part != nullptr) {
    const double s = cert_block_sum(nrm);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
  }
}

// beta_j = ||w||; breakdown test; v_{j+1} = w / beta_j. Every block sums
// the same partials in the same order, so all blocks take the same
// branch. Block 0 records beta_j and the step count and raises the flag;
// a block that already sees the flag raised by block 0 of this launch
// returns without normalising, which is what the breakdown branch does.
__global__ void k_cert_norm(const double* __restrict__ w,
                            double* __restrict__ vnext, long N,
                            double* __restrict__ cc,
                            const double* __restrict__ part, int npart,
                            int j, int m) {
  // one flag read per block: block 0 of this launch may be raising it
  // right now, and a block must not split over the two values
  __shared__ int off;
  if (threadIdx.x == 0) off = cert_off(cc) ? 1 : 0;
  __syncthreads();
  if (off) return;
  const double beta = sqrt(cert_sum_partials(part, npart));
  const bool ok = beta >= cc[CC_TOL] && beta > 0.0;  // false for NaN too
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    cc[CC_HDR + m + j] = ok ? beta : 0.0;
    cc[CC_COUNT] = (double)(j + 1);
    if (!ok) cc[CC_FLAG] = 1.0;
  }
  if (!ok) return;
  const double inv = 1.0 / beta;
  for (long row = (long)blockIdx.x * CERT_BS + threadIdx.x; row < N;
       row += (long)gridDim.x * CERT_BS)
    vnext[row] = w[row] * inv;
}

static void launch_cert_lambda(const double* X, const double* QX,
                               double* lam, double* part, int n, int d,
                               int r, hipStream_t s) {
  if (!dispatch_dr(d, r, [&](auto Dc, auto Rc) {
        hipLaunchKernelGGL((k_cert_lambda<Dc, Rc>), dim3(cert_grid(n)),
                           dim3(CERT_BS), 0, s, X, QX, lam, part, n);
      }))
    dpo_bad_shape(d, r);
}

static void launch_cert_apply(const int* rp, const int* ci,
                              const double* vals, const double* lam,
                              const double* v, const double* vprev,
                              const double* beta_prev, double* w,
                              double* part, int n, int d, const double* cc,
                              hipStream_t s) {
  const int grid = cert_grid((long)n * (d + 1));
  if (d == 2)
    hipLaunchKernelGGL((k_cert_apply<2>), dim3(grid), dim3(CERT_BS), 0, s,
                       rp, ci, vals, lam, v, vprev, beta_prev, w, part, n,
                       cc);
  else if (d == 3)
    hipLaunchKernelGGL((k_cert_apply<3>), dim3(grid), dim3(CERT_BS), 0, s,
                       rp, ci, vals, lam, v, vprev, beta_prev, w, part, n,
                       cc);
  else
    dpo_bad_shape(d, -1);
}

static void launch_cert_gram_split(const double* V, const double* w,
                                   double* c, double* gpart,
                                   const double* cc, const double* part,
                                   double* alpha_out, int ncols, long N,
                                   hipStream_t s) {
  const int grid = cert_grid(N);
  hipLaunchKernelGGL(k_cert_gram_split, dim3(grid), dim3(CERT_BS), 0, s, V,
                     w, gpart, ncols, N, cc);
  hipLaunchKernelGGL(k_cert_gram_finish, dim3(ncols), dim3(CERT_BS), 0, s,
                     (const double*)gpart, grid, c, cc, part, grid,
                     alpha_out);
}

// Lanczos steps first_step .. first_step + nsteps - 1 (below m) on the
// stream. gpart == nullptr: c = V^T w by k_cert_gram, one workgroup per
// column; otherwise by the row-split pair with gpart as its slots.
static void cert_enqueue_steps(const int* row_ptr, const int* col_idx,
                               const double* vals, const double* lam,
                               double* V, double* w, double* cvec,
                               double* part, double* gpart, double* cc,
                               int n, int d, int m, int first_step,
                               int nsteps, hipStream_t s) {
  const long N = (long)n * (d + 1);
  const int grid = cert_grid(N);
  for (int j = first_step; j < first_step + nsteps && j < m; ++j) {
    const double* vj = V + (size_t)j * N;
    const double* vp = j > 0 ? V + (size_t)(j - 1) * N : nullptr;
    const double* bp = j > 0 ? cc + CC_HDR + m + j - 1 : nullptr;
    launch_cert_apply(row_ptr, col_idx, vals, lam, vj, vp, bp, w, part, n,
                      d, cc, s);
    // CGS2: two classical Gram-Schmidt passes against columns 0..j
    for (int pass = 0; pass < 2; ++pass) {
      double* alpha_out = pass == 0 ? cc + CC_HDR + j : nullptr;
      if (gpart != nullptr)
        launch_cert_gram_split(V, w, cvec, gpart, cc, part, alpha_out,
                               j + 1, N, s);
      else
        hipLaunchKernelGGL(k_cert_gram, dim3(j + 1), dim3(CERT_BS), 0, s,
                           (const double*)V, (const double*)w, cvec, N,
                           (const double*)cc, (const double*)part, grid,
                           alpha_out);
      hipLaunchKernelGGL(k_cert_sub, dim3(grid), dim3(CERT_BS), 0, s,
                         (const double*)V, (const double*)cvec, w, j + 1, N,
                         (const double*)cc, pass == 1 ? part : nullptr);
    }
    hipLaunchKernelGGL(k_cert_norm, dim3(grid), dim3(CERT_BS), 0, s,
                       (const double*)w, V + (size_t)(j + 1) * N, N, cc,
                       (const double*)part, grid, j, m);
  }
}

extern "C" {

// lam (n, d, d) and res_out[0] = ||QX - Lambda X||_F^2 from X and
// QX = Q @ X (both (N, r)). part: CERT_MAX_PART scratch doubles.
void dpo_cert_lambda(const double* X, const double* QX, double* lam,
                     double* res_out, double* part, int n, int d, int r,
                     void* stream) {
  hipStream_t s = (hipStream_t)stream;
  launch_cert_lambda(X, QX, lam, part, n, d, r, s);
  hipLaunchKernelGGL(k_cert_reduce, dim3(1), dim3(CERT_BS), 0, s, part,
                     cert_grid(n), res_out);
}

// Stand-alone operator application: w = S v - beta_prev[0] * vprev,
// alpha_out[0] = <v, w>. vprev / beta_prev may be null.
void dpo_cert_apply(const int* row_ptr, const int* col_idx,
                    const double* vals, const double* lam, const double* v,
                    const double* vprev, const double* beta_prev, double* w,
                    double* alpha_out, double* part, int n, int d,
                    void* stream) {
  hipStream_t s = (hipStream_t)stream;
  launch_cert_apply(row_ptr, col_idx, vals, lam, v, vprev, beta_prev, w,
                    part, n, d, nullptr, s);
  hipLaunchKernelGGL(k_cert_reduce, dim3(1), dim3(CERT_BS), 0, s, part,
                     cert_grid((long)n * (d + 1)), alpha_out);
}

// Enqueue Lanczos steps first_step .. first_step + nsteps - 1 on the
// stream, eagerly and with no host synchronisation. V holds m + 1
// columns of length N (column j = v_j), cvec m + 1 doubles, part
// CERT_MAX_PART doubles, cc CC_HDR + 2 m doubles. Step j reads columns
// 0..j and writes column j + 1 <= m; steps at or past m are not enqueued.
void dpo_cert_lanczos(const int* row_ptr, const int* col_idx,
                      const double* vals, const double* lam, double* V,
                      double* w, double* cvec, double* part, double* cc,
                      int n, int d, int m, int first_step, int nsteps,
                      void* stream) {
  cert_enqueue_steps(row_ptr, col_idx, vals, lam, V, w, cvec, part,
                     nullptr, cc, n, d, m, first_step, nsteps,
                     (hipStream_t)stream);
}

// The same steps inside a thick-restart window of b = m columns, with
// the row-split Gram: gpart holds (m + 1) * CERT_MAX_PART doubles. After
// a restart that kept k Ritz vectors the host resets the step count to
// k and zeroes beta[k - 1]; step k then needs no special case.
void dpo_cert_lanczos_split(const int* row_ptr, const int* col_idx,
                            const double* vals, const double* lam,
                            double* V, double* w, double* cvec,
                            double* part, double* gpart, double* cc, int n,
                            int d, int m, int first_step, int nsteps,
                            void* stream) {
  cert_enqueue_steps(row_ptr, col_idx, vals, lam, V, w, cvec, part, gpart,
                     cc, n, d, m, first_step, nsteps, (hipStream_t)stream);
}

// Stand-alone row-split Gram: c[0..ncols) = V^T w and, with alpha_out,
// alpha_out[0] = sum of the cert_grid(N) partials in part. gpart: ncols *
// CERT_MAX_PART doubles. cc may be null (no guard).
void dpo_cert_gram_split(const double* V, const double* w, double* c,
                         double* gpart, const double* cc,
                         const double* part, double* alpha_out, int ncols,
                         long N, void* stream) {
  launch_cert_gram_split(V, w, c, gpart, cc, part, alpha_out, ncols, N,
                         (hipStream_t)stream);
}

// Thick-restart contraction V[0..k) <- C^T V[0..b), V[k] <- V[b], in
// place; C is b x CERT_KEEP_MAX row-major, zero beyond column k.
void dpo_cert_contract(double* V, const double* C, int b, int k, long N,
                       void* stream) {
  hipLaunchKernelGGL(k_cert_contract, dim3(cert_grid(N)), dim3(CERT_BS), 0,
                     (hipStream_t)stream, V, C, b, k, N);
}

int dpo_cert_ctrl_header() { return CC_HDR; }
int dpo_cert_max_part() { return CERT_MAX_PART; }
int dpo_cert_keep_max() { return CERT_KEEP_MAX; }

}  // extern "C"

// =====================================================================
// refine: device-resident global Riemannian trust region on
// f(X) = 0.5 <Q, X^T X> (docs/DESIGN.md §17). Steihaug-Toint
// preconditioned tCG with the scalar logic of solver.truncated_cg /
// trust_region batch mode, no Krylov history and no cap on the inner
// iterations: the model decrease is a scalar recurrence.
//
// Execution model of the certificate: eager launches, a control array
// `rc` of its own, every kernel guarded by rc[RF_STATUS], per-block
// partials in fixed slots summed by cert_sum_partials in the one-block
// control kernel that follows (a later launch, so the kernel boundary
// publishes them). No floating-point atomics in any refine kernel.
// Q @ V is k_bsr_spmm itself (guarded by the same slot 0).
// =====================================================================
enum RefSlot {
  RF_STATUS = 0,   // RefStatus; slot 0 so that the guards of k_bsr_spmm,
                   // k_polar_affine and k_precond_dense read it
  RF_FX = 1, RF_GN2 = 2, RF_RR = 3, RF_ZR = 4, RF_EPE = 5, RF_EPD = 6,
  RF_DPD = 7, RF_COEF = 8, RF_BETA = 9,
  RF_ITER = 10,      // Hd applications of the current tCG
  RF_RADIUS = 11, RF_BOUND = 12,
  RF_DM = 13,        // model decrease of eta (scalar recurrence)
  RF_STOP = 14,      // boundary / negative curvature met in this iteration
  RF_TCG = 15,       // RefTcg: how the last tCG ended
  RF_FPROP = 16, RF_RHO = 17, RF_ACCEPTED = 18,
  RF_GRAD_TOL = 19, RF_MAX_INNER = 20, RF_MAX_RADIUS = 21,
  RF_OUTER = 22,     // candidates evaluated
  RF_INNER = 23,     // Hd applications over all outer steps
  RF_REJECTED = 24, RF_STREAK = 25,  // rejections: total, in a row
  RF_HIT = 26,       // last tCG ended on the boundary
  RF_DHD = 27,       // last <delta, Hd>
  RF_SIZE = 32,
};
enum RefStatus { RS_RUN = 0, RS_TCG_DONE = 1, RS_CONVERGED = 2,
                 RS_HEAD = 3 };
enum RefTcg { RT_NONE = 0, RT_CONVERGED = 1, RT_EXCEEDED_TR = 2,
              RT_NEG_CURV = 3, RT_MAX_INNER = 4 };
enum RefStage { RG_HEAD = 0, RG_Z0 = 1, RG_ALPHA = 2, RG_RR = 3,
                RG_BETA = 4, RG_ACCEPT = 5 };

__device__ __forceinline__ bool ref_off(const double* rc, int status) {
  return rc[RF_STATUS] != (double)status;
}

// The scalar step between two vector kernels: one block sums the
// partials of the launch before it (s0 from part[0..np), s1 from
// part[CERT_MAX_PART..+np)) and thread 0 advances the control array.
__global__ void k_ref_ctl(double* __restrict__ rc,
                          const double* __restrict__ part, int np,
                          int stage) {
  const int want = stage == RG_HEAD ? RS_HEAD
                   : stage == RG_ACCEPT ? RS_TCG_DONE : RS_RUN;
  if (ref_off(rc, want)) return;
  const double s0 = cert_sum_partials(part, np);
  const double s1 =
      stage == RG_HEAD ? cert_sum_partials(part + CERT_MAX_PART, np) : 0.0;
  if (threadIdx.x != 0) return;
  switch (stage) {
    case RG_HEAD: {
      // s0 = <QX, X>, s1 = ||grad||^2; theta = 1, kappa = 0.1
      const double nr0 = sqrt(s1);
      rc[RF_FX] = 0.5 * s0;
      rc[RF_GN2] = s1;
      rc[RF_RR] = s1;
      rc[RF_BOUND] = nr0 * fmin(nr0, 0.1);
      rc[RF_EPE] = 0.0;
      rc[RF_EPD] = 0.0;
      rc[RF_COEF] = 0.0;
      rc[RF_BETA] = 0.0;
      rc[RF_ITER] = 0.0;
      rc[RF_DM] = 0.0;
      rc[RF_STOP] = 0.0;
      rc[RF_HIT] = 0.0;  // RF_TCG keeps the last tCG's ending
      rc[RF_STATUS] =
          nr0 <= rc[RF_GRAD_TOL] ? (double)RS_CONVERGED : (double)RS_RUN;
      break;
    }
    case RG_Z0:  // s0 = <z0, r0>
      rc[RF_ZR] = s0;
      rc[RF_DPD] = s0;
      break;
    case RG_ALPHA: {  // s0 = <delta, Hd>
      const double d_Hd = s0, z_r = rc[RF_ZR];
      const double e_Pe = rc[RF_EPE], e_Pd = rc[RF_EPD], d_Pd = rc[RF_DPD];
      const double rad2 = rc[RF_RADIUS] * rc[RF_RADIUS];
      const double alpha = z_r / d_Hd;
      const double e_Pe_new =
          e_Pe + 2.0 * alpha * e_Pd + alpha * alpha * d_Pd;
      rc[RF_DHD] = d_Hd;
      rc[RF_ITER] += 1.0;
      rc[RF_INNER] += 1.0;
      if (d_Hd <= 0.0 || e_Pe_new >= rad2) {
        const double disc = e_Pd * e_Pd + d_Pd * (rad2 - e_Pe);
        const double tau =
            d_Pd > 0.0 ? (-e_Pd + sqrt(fmax(disc, 0.0))) / d_Pd : 0.0;
        rc[RF_COEF] = tau;
        rc[RF_DM] += tau * z_r - 0.5 * tau * tau * d_Hd;
        rc[RF_STOP] = 1.0;
        rc[RF_TCG] =
            d_Hd <= 0.0 ? (double)RT_NEG_CURV : (double)RT_EXCEEDED_TR;
      } else {
        rc[RF_COEF] = alpha;
        rc[RF_EPE] = e_Pe_new;
        rc[RF_DM] += 0.5 * alpha * z_r;
      }
      break;
    }
    case RG_RR: {  // s0 = ||r||^2 unless a stop is pending
      if (rc[RF_STOP] != 0.0) {
        rc[RF_HIT] = 1.0;
        rc[RF_STATUS] = (double)RS_TCG_DONE;
        break;
      }
      rc[RF_RR] = s0;
      if (sqrt(s0) <= rc[RF_BOUND]) {
        rc[RF_TCG] = (double)RT_CONVERGED;
        rc[RF_STATUS] = (double)RS_TCG_DONE;
      } else if (rc[RF_ITER] >= rc[RF_MAX_INNER]) {
        rc[RF_TCG] = (double)RT_MAX_INNER;
        rc[RF_STATUS] = (double)RS_TCG_DONE;
      }
      break;
    }
    case RG_BETA: {  // s0 = <z, r>
      const double z_r = rc[RF_ZR], alpha = rc[RF_COEF];
      const double beta = s0 / z_r;
      rc[RF_BETA] = beta;
      rc[RF_EPD] = beta * (rc[RF_EPD] + alpha * rc[RF_DPD]);
      rc[RF_DPD] = s0 + beta * beta * rc[RF_DPD];
      rc[RF_ZR] = s0;
      break;
    }
    case RG_ACCEPT: {  // s0 = <Q Xp, Xp>
      const double fprop = 0.5 * s0, fX = rc[RF_FX];
      const double rho = (fX - fprop) / fmax(rc[RF_DM], 1e-300);
      rc[RF_FPROP] = fprop;
      rc[RF_RHO] = rho;
      if (rho < 0.25)
        rc[RF_RADIUS] *= 0.25;
      else if (rho > 0.75 && rc[RF_HIT] != 0.0)
        rc[RF_RADIUS] = fmin(2.0 * rc[RF_RADIUS], rc[RF_MAX_RADIUS]);
      const bool acc = rho > 0.1 && fprop <= fX;
      rc[RF_ACCEPTED] = acc ? 1.0 : 0.0;
      rc[RF_STREAK] = acc ? 0.0 : rc[RF_STREAK] + 1.0;
      if (!acc) rc[RF_REJECTED] += 1.0;
      rc[RF_OUTER] += 1.0;
      rc[RF_STATUS] = (double)RS_HEAD;
      break;
    }
  }
}

// Per-pose stage behind Q @ V (one thread per pose, grid capped and
// strided like the certificate's): T is the pose's tile of `in`.
//   RP_GRAD  in = Q X: part0 += <T, X>; T = P_X(T); grad = r = T,
//            eta = 0, part1 += ||T||^2
//   RP_HD    in = Q delta: Hd = P_X(T); part0 += <delta, Hd>
//   RP_Z     in = M^-1 r from the dense apply: z = P_X(T) in place;
//            part0 += <z, r>
//   RP_ZJ    T = block-Jacobi solve of r with the factors L; then RP_Z
// zero, when given, has this pose's tile cleared in front of the dense
// apply that follows.
enum RefProj { RP_GRAD = 0, RP_HD = 1, RP_Z = 2, RP_ZJ = 3 };

// Launched with CERT_BS threads only: the bound lets the wide shapes keep
// their tile in registers instead of spilling at the default 128 VGPRs.
template <int D, int R, int MODE>
__global__ void __launch_bounds__(CERT_BS) k_ref_proj(const double* __restrict__ rc, int status,
                           const double* __restrict__ X,
                           const double* in,
                           const double* __restrict__ L,
                           const double* __restrict__ dotw,
                           double* out, double* __restrict__ out2,
                           double* __restrict__ eta,
                           double* __restrict__ zero,
                           double* __restrict__ part, int n) {
  if (ref_off(rc, status)) return;
  constexpr int dh = D + 1;
  double p0 = 0.0, p1 = 0.0;
  for (int i = blockIdx.x * CERT_BS + threadIdx.x; i < n;
       i += gridDim.x * CERT_BS) {
    const size_t o = (size_t)i * dh * R;
    const double* Xi = X + o;
    double T[dh][R];
    if (MODE == RP_ZJ) {
      #pragma unroll
      for (int k = 0; k < R; ++k) {
        double y[dh];
        chol_solve_col<dh>(L + (size_t)i * dh * dh, in + o + k, R, y);
        #pragma unroll
        for (int c = 0; c < dh; ++c) T[c][k] = y[c];
      }
    } else {
      #pragma unroll
      for (int c = 0; c < dh; ++c)
        #pragma unroll
        for (int k = 0; k < R; ++k) T[c][k] = in[o + c * R + k];
    }
    if (MODE == RP_GRAD) {
      #pragma unroll
      for (int c = 0; c < dh; ++c)
        #pragma unroll
        for (int k = 0; k < R; ++k) p0 = fma(T[c][k], Xi[c * R + k], p0);
    }
    tangent_project<D, R>(Xi, T);
    #pragma unroll
    for (int c = 0; c < dh; ++c)
      #pragma unroll
      for (int k = 0; k < R; ++k) {
        const size_t e = o + c * R + k;
        const double t = T[c][k];
        out[e] = t;
        if (MODE == RP_GRAD) {
          out2[e] = t;
          eta[e] = 0.0;
          p1 = fma(t, t, p1);
        } else {
          p0 = fma(t, dotw[e], p0);
        }
        if (zero != nullptr) zero[e] = 0.0;
      }
  }
  const double s0 = cert_block_sum(p0);
  if (threadIdx.x == 0) part[blockIdx.x] = s0;
  if (MODE == RP_GRAD) {
    const double s1 = cert_block_sum(p1);
    if (threadIdx.x == 0) part[CERT_MAX_PART + blockIdx.x] = s1;
  }
}

// eta += coef * delta; unless a stop is pending r += coef * Hd with the
// block partial of ||r||^2 (and z cleared for the dense apply).
__global__ void k_ref_update(const double* __restrict__ rc,
                             double* __restrict__ eta,
                             double* __restrict__ rvec,
                             const double* __restrict__ delta,
                             const double* __restrict__ Hd,
                             double* __restrict__ zero,
                             double* __restrict__ part, long total) {
  if (ref_off(rc, RS_RUN)) return;
  const double coef = rc[RF_COEF];
  const bool stop = rc[RF_STOP] != 0.0;
  double nrm = 0.0;
  for (long e = (long)blockIdx.x * CERT_BS + threadIdx.x; e < total;
       e += (long)gridDim.x * CERT_BS) {
    eta[e] = fma(coef, delta[e], eta[e]);
    if (!stop) {
      const double rv = fma(coef, Hd[e], rvec[e]);
      rvec[e] = rv;
      nrm = fma(rv, rv, nrm);
      if (zero != nullptr) zero[e] = 0.0;
    }
  }
  const double s = cert_block_sum(nrm);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// delta = beta * delta - z; beta == 0 (the first direction of a tCG)
// does not read the old delta.
__global__ void k_ref_delta(const double* __restrict__ rc,
                            double* __restrict__ delta,
                            const double* __restrict__ z, long total) {
  if (ref_off(rc, RS_RUN)) return;
  const double beta = rc[RF_BETA];
  for (long e = (long)blockIdx.x * CERT_BS + threadIdx.x; e < total;
       e += (long)gridDim.x * CERT_BS)
    delta[e] = beta == 0.0 ? -z[e] : fma(beta, delta[e], -z[e]);
}

// part[b] = block partial of <A, B> (f of the proposal)
__global__ void k_ref_dot(const double* __restrict__ rc, int status,
                          const double* __restrict__ A,
                          const double* __restrict__ B,
                          double* __restrict__ part, long total) {
  if (ref_off(rc, status)) return;
  double dot = 0.0;
  for (long e = (long)blockIdx.x * CERT_BS + threadIdx.x; e < total;
       e += (long)gridDim.x * CERT_BS)
    dot = fma(A[e], B[e], dot);
  const double s = cert_block_sum(dot);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// X = Xp behind an accepted candidate. Enqueued again it copies the same
// values: Xp changes only in the next candidate stage.
__global__ void k_ref_copy(const double* __restrict__ rc,
                           double* __restrict__ X,
                           const double* __restrict__ Xp, long total) {
  if (ref_off(rc, RS_HEAD) || rc[RF_ACCEPTED] == 0.0) return;
  for (long e = (long)blockIdx.x * CERT_BS + threadIdx.x; e < total;
       e += (long)gridDim.x * CERT_BS)
    X[e] = Xp[e];
}

// The refine buffers, all (N, r) but part (2 * CERT_MAX_PART) and rc.
struct RefBufs {
  const int *rp, *ci;
  const double* vals;
  double *X, *Xp, *QV, *grad, *eta, *rvec, *z, *delta, *Hd;
  const double* L;     // block-Jacobi factors, or
  const float* Minv;   // the dense fp32 inverse
  double *part, *rc;
  int n, d, r;
};

static inline void ref_ctl(const RefBufs& b, int np, int stage,
                           hipStream_t s) {
  hipLaunchKernelGGL(k_ref_ctl, dim3(1), dim3(CERT_BS), 0, s, b.rc,
                     (const double*)b.part, np, stage);
}

template <int MODE>
static void ref_proj(const RefBufs& b, int status, const double* in,
                     const double* dotw, double* out, double* out2,
                     double* eta, double* zero, hipStream_t s) {
  if (!dispatch_dr(b.d, b.r, [&](auto Dc, auto Rc) {
        hipLaunchKernelGGL((k_ref_proj<Dc, Rc, MODE>),
                           dim3(cert_grid(b.n)), dim3(CERT_BS), 0, s,
                           (const double*)b.rc, status,
                           (const double*)b.X, in, b.L, dotw, out, out2,
                           eta, zero, b.part, b.n);
      }))
    dpo_bad_shape(b.d, b.r);
}

// z = P_X(M^-1 r) and the partials of <z, r> (status RS_RUN)
static void ref_precond(const RefBufs& b, hipStream_t s) {
  if (b.Minv != nullptr) {
    // z was cleared by the kernel that wrote r
    launch_precond_dense(b.Minv, b.rvec, b.z, b.n * (b.d + 1), b.r, b.rc,
                         RS_RUN, s);
    ref_proj<RP_Z>(b, RS_RUN, b.z, b.rvec, b.z, nullptr, nullptr, nullptr,
                   s);
  } else {
    ref_proj<RP_ZJ>(b, RS_RUN, b.rvec, b.rvec, b.z, nullptr, nullptr,
                    nullptr, s);
  }
}

static void ref_hd(const RefBufs& b, hipStream_t s) {
  launch_spmm(b.rp, b.ci, b.vals, b.n, b.d, b.r, b.delta, b.QV, b.rc,
              RS_RUN, s);
  ref_proj<RP_HD>(b, RS_RUN, b.QV, b.delta, b.Hd, nullptr, nullptr,
                  nullptr, s);
}

static void ref_enqueue_head(const RefBufs& b, hipStream_t s) {
  const long total = (long)b.n * (b.d + 1) * b.r;
  const int gp = cert_grid(b.n);
  launch_spmm(b.rp, b.ci, b.vals, b.n, b.d, b.r, b.X, b.QV, b.rc, RS_HEAD,
              s);
  ref_proj<RP_GRAD>(b, RS_HEAD, b.QV, nullptr, b.grad, b.rvec, b.eta,
                    b.Minv != nullptr ? b.z : nullptr, s);
  ref_ctl(b, gp, RG_HEAD, s);
  ref_precond(b, s);
  ref_ctl(b, gp, RG_Z0, s);
  hipLaunchKernelGGL(k_ref_delta, dim3(cert_grid(total)), dim3(CERT_BS), 0,
                     s, (const double*)b.rc, b.delta, (const double*)b.z,
                     total);
}

static void ref_enqueue_tcg(const RefBufs& b, int nsteps, hipStream_t s) {
  const long total = (long)b.n * (b.d + 1) * b.r;
  const int gp = cert_grid(b.n), ge = cert_grid(total);
  for (int it = 0; it < nsteps; ++it) {
    ref_hd(b, s);
    ref_ctl(b, gp, RG_ALPHA, s);
    hipLaunchKernelGGL(k_ref_update, dim3(ge), dim3(CERT_BS), 0, s,
                       (const double*)b.rc, b.eta, b.rvec,
                       (const double*)b.delta, (const double*)b.Hd,
                       b.Minv != nullptr ? b.z : nullptr, b.part, total);
    ref_ctl(b, ge, RG_RR, s);
    ref_precond(b, s);
    ref_ctl(b, gp, RG_BETA, s);
    hipLaunchKernelGGL(k_ref_delta, dim3(ge), dim3(CERT_BS), 0, s,
                       (const double*)b.rc, b.delta, (const double*)b.z,
                       total);
  }
}

static void ref_enqueue_candidate(const RefBufs& b, hipStream_t s) {
  const long total = (long)b.n * (b.d + 1) * b.r;
  const int ge = cert_grid(total);
  launch_polar(b.X, b.eta, nullptr, 1.0, 1.0, 0.0, b.Xp, b.n, b.d, b.r,
               b.rc, RS_TCG_DONE, s);
  launch_spmm(b.rp, b.ci, b.vals, b.n, b.d, b.r, b.Xp, b.QV, b.rc,
              RS_TCG_DONE, s);
  hipLaunchKernelGGL(k_ref_dot, dim3(ge), dim3(CERT_BS), 0, s,
                     (const double*)b.rc, (int)RS_TCG_DONE,
                     (const double*)b.QV, (const double*)b.Xp, b.part,
                     total);
  ref_ctl(b, ge, RG_ACCEPT, s);
  hipLaunchKernelGGL(k_ref_copy, dim3(ge), dim3(CERT_BS), 0, s,
                     (const double*)b.rc, b.X, (const double*)b.Xp, total);
}

extern "C" {

// stage: 0 head, 1 nsteps tCG iterations, 2 candidate, 3 the Hd stage
// alone (Q delta, projection, partials; no control step). bufs: the nine
// (N, r) vectors X, Xp, QV, grad, eta, r, z, delta, Hd. Exactly one of L
// and Minv is given. Nothing synchronises.
void dpo_refine_stage(int stage, const int* row_ptr, const int* col_idx,
                      const double* vals, double* const* bufs,
                      const double* L, const float* Minv, double* part,
                      double* rc, int n, int d, int r, int nsteps,
                      void* stream) {
  RefBufs b{row_ptr, col_idx, vals,    bufs[0], bufs[1], bufs[2], bufs[3],
            bufs[4], bufs[5], bufs[6], bufs[7], bufs[8], L,       Minv,
            part,    rc,      n,       d,       r};
  hipStream_t s = (hipStream_t)stream;
  if (stage == 0) ref_enqueue_head(b, s);
  else if (stage == 1) ref_enqueue_tcg(b, nsteps, s);
  else if (stage == 2) ref_enqueue_candidate(b, s);
  else ref_hd(b, s);
}

int dpo_refine_ctrl_size() { return RF_SIZE; }

}  // extern "C"

// =====================================================================
// Rounding: the lifted iterate to SE(d) on the device (docs/DESIGN.md
// §19). Purely additive; one thread per pose, everything in registers,
// the launch geometry of k_polar_affine (per-pose maps) and
// k_cert_lambda (reductions).
//
//   k_round_gram         S = sum_i Y_i Y_i^T (r x r) over the rotation
//                        rows, per-block partials in a fixed order
//   k_round_gram_finish  sums the <= CERT_MAX_PART partials per entry
//   k_round_poses        B_i = U^T Y_i, R_i = argmax_{SO(d)} tr(R^T B_i),
//                        t_i = U^T p_i - t0, in both output layouts
//   k_round_reflections  number of poses with det(U^T Y_i) < 0
//   k_round_gauge        R_i <- R_a^T R_i, t_i <- R_a^T (t_i - t_a)
//
// Reductions follow the certificate's rule: one partial
// per block and entry, summed by a later launch in a fixed order; no
// floating-point atomics, so S is bitwise run-to-run reproducible.
//
// Projection onto SO(d). The block is first scaled by an exact power of
// two so that its largest entry lies in [1, 2): nothing is squared at
// the input's scale. d = 2: tr(R^T B) = cos(a) (B00 + B11) + sin(a)
// (B10 - B01), maximised in closed form. d = 3: tr(R(q)^T B) = q^T K q
// for the 4 x 4 symmetric Davenport matrix K, which is LINEAR in B; its
// top eigenvector comes from a fixed number of cyclic Jacobi sweeps and
// gives the rotation as a unit quaternion. The eigenvalue gap of K is
// 2 (sigma_2 + sign(det B) sigma_3), the conditioning of the problem
// itself; det B < 0, repeated singular values and singular blocks need
// no special case (any top eigenvector is a maximiser; K = 0 gives the
// identity).
// =====================================================================
#define ROUND_JACOBI_SWEEPS 8
#define ROUND_MAX_GRAM (DPO_MAX_R * (DPO_MAX_R + 1) / 2)

template <int D>
__device__ __forceinline__ void round_normalize(double (&B)[D][D]) {
  double m = 0.0;
  #pragma unroll
  for (int a = 0; a < D; ++a)
    #pragma unroll
    for (int b = 0; b < D; ++b) m = fmax(m, fabs(B[a][b]));
  if (m > 0.0 && m <= 1.7976931348623157e308) {
    const int e = -ilogb(m);
    #pragma unroll
    for (int a = 0; a < D; ++a)
      #pragma unroll
      for (int b = 0; b < D; ++b) B[a][b] = scalbn(B[a][b], e);
  }
}

// determinant of a block already normalised by round_normalize
__device__ __forceinline__ double round_det(const double (&B)[2][2]) {
  return B[0][0] * B[1][1] - B[0][1] * B[1][0];
}
__device__ __forceinline__ double round_det(const double (&B)[3][3]) {
  return B[0][0] * (B[1][1] * B[2][2] - B[1][2] * B[2][1])
       - B[0][1] * (B[1][0] * B[2][2] - B[1][2] * B[2][0])
       + B[0][2] * (B[1][0] * B[2][1] - B[1][1] * B[2][0]);
}

__device__ __forceinline__ void round_project(double (&B)[2][2],
                                              double (&Rm)[2][2]) {
  round_normalize<2>(B);
  const double x = B[0][0] + B[1][1], y = B[1][0] - B[0][1];
  const double n2 = x * x + y * y;
  const bool ok = n2 > 0.0;
  const double inv = 1.0 / sqrt(ok ? n2 : 1.0);
  const double c = ok ? x * inv : 1.0, s = ok ? y * inv : 0.0;
  Rm[0][0] = c; Rm[0][1] = -s;
  Rm[1][0] = s; Rm[1][1] = c;
}

__device__ __forceinline__ void round_project(double (&B)[3][3],
                                              double (&Rm)[3][3]) {
  round_normalize<3>(B);
  // q = (w, x, y, z); K from the expansion of sum_ij R(q)_ij B_ij
  double A[4][4], V[4][4];
  A[0][0] = B[0][0] + B[1][1] + B[2][2];
  A[1][1] = B[0][0] - B[1][1] - B[2][2];
  A[2][2] = -B[0][0] + B[1][1] - B[2][2];
  A[3][3] = -B[0][0] - B[1][1] + B[2][2];
  A[0][1] = A[1][0] = B[2][1] - B[1][2];
  A[0][2] = A[2][0] = B[0][2] - B[2][0];
  A[0][3] = A[3][0] = B[1][0] - B[0][1];
  A[1][2] = A[2][1] = B[0][1] + B[1][0];
  A[1][3] = A[3][1] = B[0][2] + B[2][0];
  A[2][3] = A[3][2] = B[1][2] + B[2][1];
  #pragma unroll
  for (int a = 0; a < 4; ++a)
    #pragma unroll
    for (int b = 0; b < 4; ++b) V[a][b] = (a == b) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < ROUND_JACOBI_SWEEPS; ++sweep) {
    #pragma unroll
    for (int p = 0; p < 3; ++p)
      #pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p][q];
        const bool nz = apq != 0.0;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * (nz ? apq : 1.0));
        // theta^2 may overflow to inf: t = 0 then, the right limit
        const double tt = copysign(1.0, theta)
                        / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double t = nz ? tt : 0.0;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        A[p][p] -= t * apq;
        A[q][q] += t * apq;
        A[p][q] = A[q][p] = 0.0;
        #pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k != p && k != q) {
            const double akp = A[k][p], akq = A[k][q];
            A[k][p] = A[p][k] = c * akp - s * akq;
            A[k][q] = A[q][k] = s * akp + c * akq;
          }
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  // eigenvector of the largest eigenvalue (ties: the first)
  double lam = A[0][0];
  double q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
  #pragma unroll
  for (int j = 1; j < 4; ++j) {
    const bool up = A[j][j] > lam;
    lam = up ? A[j][j] : lam;
    #pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = up ? V[k][j] : q[k];
  }
  const double inv = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]
                                + q[3] * q[3]);
  const double w = q[0] * inv, x = q[1] * inv, y = q[2] * inv,
               z = q[3] * inv;
  Rm[0][0] = 1.0 - 2.0 * (y * y + z * z);
  Rm[0][1] = 2.0 * (x * y - w * z);
  Rm[0][2] = 2.0 * (x * z + w * y);
  Rm[1][0] = 2.0 * (x * y + w * z);
  Rm[1][1] = 1.0 - 2.0 * (x * x + z * z);
  Rm[1][2] = 2.0 * (y * z - w * x);
  Rm[2][0] = 2.0 * (x * z - w * y);
  Rm[2][1] = 2.0 * (y * z + w * x);
  Rm[2][2] = 1.0 - 2.0 * (x * x + y * y);
}

// B[c][a] = sum_k sg_c U[k][c] Y[k][a] of pose block Xi (Xt layout:
// Xi[a * R + k] = Y[k][a]); U is (R, D) row-major, sg_c = -1 on the
// last column when flip is set
template <int D, int R>
__device__ __forceinline__ void round_block(const double* __restrict__ Xi,
                                            const double* __restrict__ U,
                                            int flip, double (&B)[D][D]) {
  #pragma unroll
  for (int c = 0; c < D; ++c) {
    const double sg = (flip && c == D - 1) ? -1.0 : 1.0;
    #pragma unroll
    for (int a = 0; a < D; ++a) {
      double s = 0.0;
      #pragma unroll
      for (int k = 0; k < R; ++k) s = fma(U[k * D + c], Xi[a * R + k], s);
      B[c][a] = sg * s;
    }
  }
}

template <int D, int R>
__global__ void __launch_bounds__(CERT_BS)
k_round_gram(const double* __restrict__ X, double* __restrict__ gpart,
             int n) {
  constexpr int dh = D + 1;
  constexpr int NE = R * (R + 1) / 2;
  double acc[NE];
  #pragma unroll
  for (int e = 0; e < NE; ++e) acc[e] = 0.0;
  for (int i = blockIdx.x * CERT_BS + threadIdx.x; i < n;
       i += gridDim.x * CERT_BS) {
    const double* Xi = X + (size_t)i * dh * R;
    double Y[D][R];
    #pragma unroll
    for (int a = 0; a < D; ++a)
      #pragma unroll
      for (int k = 0; k < R; ++k) Y[a][k] = Xi[a * R + k];
    int e = 0;
    #pragma unroll
    for (int k = 0; k < R; ++k)
      #pragma unroll
      for (int l = k; l < R; ++l, ++e) {
        double s = acc[e];
        #pragma unroll
        for (int a = 0; a < D; ++a) s = fma(Y[a][k], Y[a][l], s);
        acc[e] = s;
      }
  }
  #pragma unroll
  for (int e = 0; e < NE; ++e) {
    const double s = cert_block_sum(acc[e]);
    if (threadIdx.x == 0) gpart[e * CERT_MAX_PART + blockIdx.x] = s;
  }
}

// S (r, r) row-major, both triangles, from the per-block partials
__global__ void __launch_bounds__(CERT_BS)
k_round_gram_finish(const double* __restrict__ gpart, int npart, int r,
                    double* __restrict__ S) {
  int e = 0;
  for (int k = 0; k < r; ++k)
    for (int l = k; l < r; ++l, ++e) {
      const double s = cert_sum_partials(gpart + e * CERT_MAX_PART, npart);
      if (threadIdx.x == 0) {
        S[k * r + l] = s;
        S[l * r + k] = s;
      }
    }
}

template <int D, int R>
__global__ void k_round_poses(const double* __restrict__ X,
                              const double* __restrict__ U,
                              const double* __restrict__ t0, int flip,
                              double* __restrict__ traj,
                              double* __restrict__ Xr, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int dh = D + 1;
  const double* Xi = X + (size_t)i * dh * R;
  double B[D][D], Rm[D][D], t[D];
  round_block<D, R>(Xi, U, flip, B);
  #pragma unroll
  for (int c = 0; c < D; ++c) {
    const double sg = (flip && c == D - 1) ? -1.0 : 1.0;
    double s = 0.0;
    #pragma unroll
    for (int k = 0; k < R; ++k) s = fma(U[k * D + c], Xi[D * R + k], s);
    t[c] = sg * s - t0[c];
  }
  round_project(B, Rm);
  const size_t ld = (size_t)n * dh;
  double* Ti = traj + (size_t)i * dh;
  double* Xo = Xr + (size_t)i * dh * D;
  #pragma unroll
  for (int c = 0; c < D; ++c) {
    #pragma unroll
    for (int a = 0; a < D; ++a) {
      Ti[c * ld + a] = Rm[c][a];
      Xo[a * D + c] = Rm[c][a];
    }
    Ti[c * ld + D] = t[c];
    Xo[D * D + c] = t[c];
  }
}

// fixed-order block sum of an int (blockDim.x == CERT_BS)
__device__ __forceinline__ int round_block_count(int v) {
  __shared__ int shc[CERT_BS / 64];
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) shc[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = shc[0];
  #pragma unroll
  for (int w = 1; w < CERT_BS / 64; ++w) s += shc[w];
  __syncthreads();
  return s;
}

template <int D, int R>
__global__ void __launch_bounds__(CERT_BS)
k_round_reflections(const double* __restrict__ X,
                    const double* __restrict__ U, int* __restrict__ ipart,
                    int n) {
  constexpr int dh = D + 1;
  int cnt = 0;
  for (int i = blockIdx.x * CERT_BS + threadIdx.x; i < n;
       i += gridDim.x * CERT_BS) {
    double B[D][D];
    round_block<D, R>(X + (size_t)i * dh * R, U, 0, B);
    round_normalize<D>(B);
    cnt += round_det(B) < 0.0 ? 1 : 0;
  }
  const int s = round_block_count(cnt);
  if (threadIdx.x == 0) ipart[blockIdx.x] = s;
}

__global__ void __launch_bounds__(CERT_BS)
k_round_count_finish(const int* __restrict__ ipart, int npart,
                     int* __restrict__ count) {
  const int t = threadIdx.x;
  const int s = round_block_count(t < npart ? ipart[t] : 0);
  if (t == 0) count[0] = s;
}

// anchor: one pose block in the Xt layout at rank d ((d + 1) x d: rows
// a < d hold R_a[:, a], row d holds t_a), in a buffer of its own (the
// pose it was copied from is overwritten like every other)
template <int D>
__global__ void k_round_gauge(double* __restrict__ Xr,
                              double* __restrict__ traj,
                              const double* __restrict__ anchor, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int dh = D + 1;
  double* Xo = Xr + (size_t)i * dh * D;
  double P[dh][D];
  #pragma unroll
  for (int a = 0; a < dh; ++a)
    #pragma unroll
    for (int k = 0; k < D; ++k) P[a][k] = Xo[a * D + k];
  #pragma unroll
  for (int k = 0; k < D; ++k) P[D][k] -= anchor[D * D + k];
  const size_t ld = (size_t)n * dh;
  double* Ti = traj + (size_t)i * dh;
  #pragma unroll
  for (int a = 0; a < dh; ++a)
    #pragma unroll
    for (int c = 0; c < D; ++c) {
      // (R_a^T v)[c] = sum_k R_a[k][c] v[k], R_a[k][c] = anchor[c * D + k]
      double s = 0.0;
      #pragma unroll
      for (int k = 0; k < D; ++k) s = fma(anchor[c * D + k], P[a][k], s);
      Xo[a * D + c] = s;
      Ti[c * ld + a] = s;
    }
}

extern "C" {

// S (r, r) = sum_i Y_i Y_i^T. gpart: dpo_round_gram_part() scratch
// doubles. Nothing synchronises.
void dpo_round_gram(const double* X, double* S, double* gpart, int n, int d,
                    int r, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int g = cert_grid(n);
  if (!dispatch_dr(d, r, [&](auto Dc, auto Rc) {
        hipLaunchKernelGGL((k_round_gram<Dc, Rc>), dim3(g), dim3(CERT_BS), 0,
                           s, X, gpart, n);
      }))
    dpo_bad_shape(d, r);
  hipLaunchKernelGGL(k_round_gram_finish, dim3(1), dim3(CERT_BS), 0, s,
                     (const double*)gpart, g, r, S);
}

int dpo_round_gram_part() { return ROUND_MAX_GRAM * CERT_MAX_PART; }

// traj (d, n (d + 1)) and Xr (n (d + 1), d) from X (n (d + 1), r), the
// basis U (r, d), the offset t0 (d) and the last-column flip
void dpo_round_poses(const double* X, const double* U, const double* t0,
                     int flip, double* traj, double* Xr, int n, int d, int r,
                     void* stream) {
  if (!dispatch_dr(d, r, [&](auto Dc, auto Rc) {
        hipLaunchKernelGGL((k_round_poses<Dc, Rc>), dim3(blocks_for(n, 256)),
                           dim3(256), 0, (hipStream_t)stream, X, U, t0, flip,
                           traj, Xr, n);
      }))
    dpo_bad_shape(d, r);
}

// count[0] = #{i : det(U^T Y_i) < 0}. ipart: CERT_MAX_PART scratch ints.
void dpo_round_reflections(const double* X, const double* U, int* count,
                           int* ipart, int n, int d, int r, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int g = cert_grid(n);
  if (!dispatch_dr(d, r, [&](auto Dc, auto Rc) {
        hipLaunchKernelGGL((k_round_reflections<Dc, Rc>), dim3(g),
                           dim3(CERT_BS), 0, s, X, U, ipart, n);
      }))
    dpo_bad_shape(d, r);
  hipLaunchKernelGGL(k_round_count_finish, dim3(1), dim3(CERT_BS), 0, s,
                     (const int*)ipart, g, count);
}

// in place on both layouts; anchor: (d + 1) x d block, not inside Xr
void dpo_round_gauge(double* Xr, double* traj, const double* anchor, int n,
                     int d, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const dim3 g(blocks_for(n, 256)), b(256);
  if (d == 2)
    hipLaunchKernelGGL(k_round_gauge<2>, g, b, 0, s, Xr, traj, anchor, n);
  else if (d == 3)
    hipLaunchKernelGGL(k_round_gauge<3>, g, b, 0, s, Xr, traj, anchor, n);
  else
    dpo_bad_shape(d, d);
}

}  // extern "C"

// =====================================================================
// Certificate, second eigensolver: LOBPCG with a Gram-based
// Rayleigh-Ritz step (docs/DESIGN.md §20). Blocks are row-major (N, m)
// like Xt, m one of the compiled r, so k_precond_dense<m> and
// k_precond_jacobi serve unchanged. B = [X W P] and SB = [SX SW SP] are
// three contiguous (N, m) blocks each.
//
// One iteration on the device: k_lob_resid (R = SX - X diag(theta),
// clears W for the dense apply), the preconditioner W = T R,
// k_lob_apply (SW = Q W - Lambda W), k_lob_gram + k_lob_gram_finish
// (B^T B, B^T SB and the m squared residual norms into `out`). The host
// reads `out`, solves the (3m) x (3m) pencil and uploads theta and the
// coefficients into the control array; k_lob_update forms the new X, P,
// SX, SP in place.
//
// House rules of the certificate section: CERT_BS threads, cert_grid,
// per-block partials in fixed slots summed by cert_sum_partials in a
// later launch, no floating-point atomics in any kernel here. Control
// array `lc`: status in slot 0 (0 = run; anything else turns every
// kernel, the reused preconditioner kernels included, into a no-op).
// =====================================================================
enum LobSlot {
  LB_STATUS = 0,
  LB_THETA = 4,    // theta[j] at LB_THETA + j, j < LOB_MAX_M
  LB_COEF = 12,    // (3m) x (2m) row-major: columns [0, m) give the new
                   // X, columns [m, 2m) the new P (rows [0, m) unused)
  LB_SIZE = 12 + 24 * 16,
};
#define LOB_MAX_M DPO_MAX_R
#define LOB_GT 4     // columns of the right operand per Gram tile
#define LOB_PAIRS 6  // block pairs (p <= q) of a 3 x 3 block matrix
// Gram tiles: 2 matrices x LOB_PAIRS x ceil(m / LOB_GT) chunks, each with
// m x LOB_GT accumulators (at most 32) and one partial per block
#define LOB_MAX_TILES (2 * LOB_PAIRS * ((LOB_MAX_M + LOB_GT - 1) / LOB_GT))
#define LOB_GPART (LOB_MAX_TILES * LOB_MAX_M * LOB_GT * CERT_MAX_PART)
#define LOB_RPART (LOB_MAX_M * CERT_MAX_PART)

__device__ __forceinline__ bool lob_off(const double* lc) {
  return lc[LB_STATUS] != 0.0;
}

// R = SX - X diag(theta), one thread per row; rpart[j * grid + block] =
// block partial of ||R[:, j]||^2. zero != nullptr: that (N, m) block is
// cleared in front of k_precond_dense.
template <int M>
__global__ void __launch_bounds__(CERT_BS)
k_lob_resid(const double* __restrict__ lc, const double* __restrict__ X,
            const double* __restrict__ SX, double* __restrict__ R,
            double* __restrict__ zero, double* __restrict__ rpart, long N) {
  if (lob_off(lc)) return;
  double th[M], nrm[M];
  #pragma unroll
  for (int j = 0; j < M; ++j) {
    th[j] = lc[LB_THETA + j];
    nrm[j] = 0.0;
  }
  for (long row = (long)blockIdx.x * CERT_BS + threadIdx.x; row < N;
       row += (long)gridDim.x * CERT_BS) {
    const size_t o = (size_t)row * M;
    #pragma unroll
    for (int j = 0; j < M; ++j) {
      const double rv = fma(-th[j], X[o + j], SX[o + j]);
      R[o + j] = rv;
      nrm[j] = fma(rv, rv, nrm[j]);
      if (zero != nullptr) zero[o + j] = 0.0;
    }
  }
  #pragma unroll
  for (int j = 0; j < M; ++j) {
    const double s = cert_block_sum(nrm[j]);
    if (threadIdx.x == 0) rpart[(size_t)j * gridDim.x + blockIdx.x] = s;
  }
}

// SW = Q W - Lambda W for M columns in one pass: the BSR traversal of
// k_bsr_spmm (one thread per element of a pose's (D+1) x M tile, grid
// stride over poses) and the d x d Lambda correction of k_cert_apply.
template <int D, int M>
__global__ void __launch_bounds__(CERT_BS)
k_lob_apply(const double* __restrict__ lc, const int* __restrict__ row_ptr,
            const int* __restrict__ col_idx, const double* __restrict__ vals,
            const double* __restrict__ lam, const double* __restrict__ W,
            double* __restrict__ SW, int n) {
  if (lob_off(lc)) return;
  constexpr int DH = D + 1;
  constexpr int tile = DH * M;
  constexpr int per_block = CERT_BS / tile;
  const int slot = threadIdx.x / tile;
  const int t = threadIdx.x % tile;
  if (slot >= per_block) return;
  const int c = t / M;  // row inside the pose block
  const int k = t % M;  // column of W
  for (long i = (long)blockIdx.x * per_block + slot; i < n;
       i += (long)gridDim.x * per_block) {
    const int s = row_ptr[i], e = row_ptr[i + 1];
    double acc = 0.0;
    for (int p = s; p < e; ++p) {
      const double* Bq = vals + (size_t)p * DH * DH + c * DH;
      const double* Wj = W + (size_t)col_idx[p] * tile;
      #pragma unroll
      for (int cc = 0; cc < DH; ++cc) acc = fma(Bq[cc], Wj[cc * M + k], acc);
    }
    if (c < D) {
      const double* Li = lam + (size_t)i * D * D + c * D;
      const double* Wi = W + (size_t)i * tile;
      #pragma unroll
      for (int b = 0; b < D; ++b) acc = fma(-Li[b], Wi[b * M + k], acc);
    }
    SW[(size_t)i * tile + c * M + k] = acc;
  }
}

// Block pair (p <= q) number `pair` of the upper block triangle.
__device__ __forceinline__ void lob_pair(int pair, int& p, int& q) {
  p = pair < 3 ? 0 : (pair < 5 ? 1 : 2);
  q = pair < 3 ? pair : (pair < 5 ? pair - 2 : 2);
}

// Row-split Gram tiles of G_B = B^T B (which = 0) and G_A = B^T SB
// (which = 1). blockIdx.y = (which * LOB_PAIRS + pair) * NCH + chunk
// selects the M x LOB_GT tile: all M columns of block p against columns
// [chunk * LOB_GT, +LOB_GT) of block q of B or SB. A tail chunk clamps
// the column and the finish kernel discards the duplicates. One partial
// per (tile entry, block) at gpart[((y * M + a) * LOB_GT + c) * grid + b].
template <int M>
__global__ void __launch_bounds__(CERT_BS)
k_lob_gram(const double* __restrict__ lc, const double* __restrict__ B,
           const double* __restrict__ SB, double* __restrict__ gpart,
           long N) {
  if (lob_off(lc)) return;
  constexpr int NCH = (M + LOB_GT - 1) / LOB_GT;
  const int y = blockIdx.y;
  const int chunk = y % NCH;
  const int which = y / (NCH * LOB_PAIRS);
  int p, q;
  lob_pair((y / NCH) % LOB_PAIRS, p, q);
  const double* L = B + (size_t)p * N * M;
  const double* Rt = (which ? SB : B) + (size_t)q * N * M;
  int col[LOB_GT];
  #pragma unroll
  for (int c = 0; c < LOB_GT; ++c) {
    const int cc = chunk * LOB_GT + c;
    col[c] = cc < M ? cc : M - 1;
  }
  double acc[M][LOB_GT];
  #pragma unroll
  for (int a = 0; a < M; ++a)
    #pragma unroll
    for (int c = 0; c < LOB_GT; ++c) acc[a][c] = 0.0;
  for (long row = (long)blockIdx.x * CERT_BS + threadIdx.x; row < N;
       row += (long)gridDim.x * CERT_BS) {
    const size_t o = (size_t)row * M;
    double rv[LOB_GT];
    #pragma unroll
    for (int c = 0; c < LOB_GT; ++c) rv[c] = Rt[o + col[c]];
    #pragma unroll
    for (int a = 0; a < M; ++a) {
      const double lv = L[o + a];
      #pragma unroll
      for (int c = 0; c < LOB_GT; ++c) acc[a][c] = fma(lv, rv[c], acc[a][c]);
    }
  }
  #pragma unroll
  for (int a = 0; a < M; ++a)
    #pragma unroll
    for (int c = 0; c < LOB_GT; ++c) {
      const double s = cert_block_sum(acc[a][c]);
      if (threadIdx.x == 0)
        gpart[((size_t)(y * M + a) * LOB_GT + c) * gridDim.x + blockIdx.x] =
            s;
    }
}

// One workgroup per Gram tile entry, then one per residual column: the
// fixed-order sum of its ngrid partials. out: G_B (3m x 3m, row-major),
// G_A (the same), then the m squared residual norms. Only entries
// (row, col) of block pairs p <= q are written: the upper triangles are
// complete, the rest of `out` is left as it was.
__global__ void __launch_bounds__(CERT_BS)
k_lob_gram_finish(const double* __restrict__ lc,
                  const double* __restrict__ gpart,
                  const double* __restrict__ rpart, int ngrid, int m,
                  double* __restrict__ out) {
  if (lob_off(lc)) return;
  const int nslot = (int)gridDim.x - m;
  const int b = blockIdx.x;
  const int k3 = 3 * m;
  if (b >= nslot) {
    const int j = b - nslot;
    const double s = cert_sum_partials(rpart + (size_t)j * ngrid, ngrid);
    if (threadIdx.x == 0) out[2 * k3 * k3 + j] = s;
    return;
  }
  const int nch = (m + LOB_GT - 1) / LOB_GT;
  const int c = b % LOB_GT;
  const int a = (b / LOB_GT) % m;
  const int y = b / (LOB_GT * m);
  const int cc = (y % nch) * LOB_GT + c;
  if (cc >= m) return;  // clamped duplicate of a tail chunk
  const int which = y / (nch * LOB_PAIRS);
  int p, q;
  lob_pair((y / nch) % LOB_PAIRS, p, q);
  const double s = cert_sum_partials(gpart + (size_t)b * ngrid, ngrid);
  if (threadIdx.x == 0)
    out[which * k3 * k3 + (p * m + a) * k3 + q * m + cc] = s;
}

// In-place update with the coefficients C at lc + LB_COEF, one thread per
// row: X <- [X W P] C[:, :M], P <- [W P] C[M:, M:], and SX, SP from SB
// with the same coefficients. A thread loads all 3M values of B and of SB
// of its row before its first store and no other thread touches that
// row, so in place is safe (the k_cert_contract argument). B and SB are
// deliberately not __restrict__: the stores alias the loads.
template <int M>
__global__ void __launch_bounds__(CERT_BS)
k_lob_update(const double* __restrict__ lc, double* B, double* SB, long N) {
  if (lob_off(lc)) return;
  const double* __restrict__ C = lc + LB_COEF;
  const size_t blk = (size_t)N * M;
  for (long row = (long)blockIdx.x * CERT_BS + threadIdx.x; row < N;
       row += (long)gridDim.x * CERT_BS) {
    const size_t o = (size_t)row * M;
    double b[3 * M], sb[3 * M];
    #pragma unroll
    for (int g = 0; g < 3; ++g)
      #pragma unroll
      for (int j = 0; j < M; ++j) {
        b[g * M + j] = B[g * blk + o + j];
        sb[g * M + j] = SB[g * blk + o + j];
      }
    #pragma unroll
    for (int j = 0; j < M; ++j) {
      double x = 0.0, sx = 0.0, pn = 0.0, sp = 0.0;
      #pragma unroll
      for (int k = 0; k < 3 * M; ++k) {
        const double cx = C[k * 2 * M + j];
        x = fma(cx, b[k], x);
        sx = fma(cx, sb[k], sx);
        if (k >= M) {
          const double cp = C[k * 2 * M + M + j];
          pn = fma(cp, b[k], pn);
          sp = fma(cp, sb[k], sp);
        }
      }
      B[o + j] = x;
      SB[o + j] = sx;
      B[2 * blk + o + j] = pn;
      SB[2 * blk + o + j] = sp;
    }
  }
}

static void lob_bad_block(int m) {
  fprintf(stderr, "dpo_ops: unsupported LOBPCG block size m=%d\n", m);
  abort();
}

static void launch_lob_resid(const double* lc, const double* X,
                             const double* SX, double* R, double* zero,
                             double* rpart, long N, int m, hipStream_t s) {
  if (!dispatch_r(m, [&](auto Mc) {
        hipLaunchKernelGGL((k_lob_resid<Mc>), dim3(cert_grid(N)),
                           dim3(CERT_BS), 0, s, lc, X, SX, R, zero, rpart,
                           N);
      }))
    lob_bad_block(m);
}

static void launch_lob_apply(const double* lc, const int* rp, const int* ci,
                             const double* vals, const double* lam,
                             const double* W, double* SW, int n, int d,
                             int m, hipStream_t s) {
  const int per_block = CERT_BS / ((d + 1) * m);
  const int grid = cert_grid((long)blocks_for(n, per_block) * CERT_BS);
  if (!dispatch_dr(d, m, [&](auto Dc, auto Mc) {
        hipLaunchKernelGGL((k_lob_apply<Dc, Mc>), dim3(grid), dim3(CERT_BS),
                           0, s, lc, rp, ci, vals, lam, W, SW, n);
      }))
    dpo_bad_shape(d, m);
}

static void launch_lob_gram(const double* lc, const double* B,
                            const double* SB, double* gpart,
                            const double* rpart, double* out, long N, int m,
                            hipStream_t s) {
  const int grid = cert_grid(N);
  const int tiles = 2 * LOB_PAIRS * ((m + LOB_GT - 1) / LOB_GT);
  if (!dispatch_r(m, [&](auto Mc) {
        hipLaunchKernelGGL((k_lob_gram<Mc>), dim3(grid, tiles),
                           dim3(CERT_BS), 0, s, lc, B, SB, gpart, N);
      }))
    lob_bad_block(m);
  hipLaunchKernelGGL(k_lob_gram_finish, dim3(tiles * m * LOB_GT + m),
                     dim3(CERT_BS), 0, s, lc, (const double*)gpart, rpart,
                     grid, m, out);
}

extern "C" {

int dpo_cert_lobpcg_ctrl_size() { return LB_SIZE; }
// doubles of the partial-slot workspace: Gram slots, then residual slots
int dpo_cert_lobpcg_part_size() { return LOB_GPART + LOB_RPART; }

// R = SX - X diag(theta); residual partials into part's residual slots.
// zero may be null.
void dpo_cert_lobpcg_resid(const double* lc, const double* X,
                           const double* SX, double* R, double* zero,
                           double* part, long N, int m, void* stream) {
  launch_lob_resid(lc, X, SX, R, zero, part + LOB_GPART, N, m,
                   (hipStream_t)stream);
}

// SW = (Q - Lambda) W for one (N, m) block
void dpo_cert_lobpcg_apply(const double* lc, const int* row_ptr,
                           const int* col_idx, const double* vals,
                           const double* lam, const double* W, double* SW,
                           int n, int d, int m, void* stream) {
  launch_lob_apply(lc, row_ptr, col_idx, vals, lam, W, SW, n, d, m,
                   (hipStream_t)stream);
}

// out = [G_B, G_A, residual norms^2] from B, SB (3 blocks each) and the
// residual slots k_lob_resid left in part
void dpo_cert_lobpcg_gram(const double* lc, const double* B,
                          const double* SB, double* part, double* out,
                          long N, int m, void* stream) {
  launch_lob_gram(lc, B, SB, part, part + LOB_GPART, out, N, m,
                  (hipStream_t)stream);
}

void dpo_cert_lobpcg_update(const double* lc, double* B, double* SB, long N,
                            int m, void* stream) {
  if (!dispatch_r(m, [&](auto Mc) {
        hipLaunchKernelGGL((k_lob_update<Mc>), dim3(cert_grid(N)),
                           dim3(CERT_BS), 0, (hipStream_t)stream, lc, B, SB,
                           N);
      }))
    lob_bad_block(m);
}

// The device half of one iteration: residual, W = T R with exactly one
// of L (block-Jacobi factors) and Minv (dense fp32 inverse), SW = S W,
// both Gram matrices. Nothing synchronises.
void dpo_cert_lobpcg_iter(const double* lc, const int* row_ptr,
                          const int* col_idx, const double* vals,
                          const double* lam, double* B, double* SB,
                          double* R, const double* L, const float* Minv,
                          double* part, double* out, int n, int d, int m,
                          void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const long N = (long)n * (d + 1);
  double* W = B + (size_t)N * m;
  double* SW = SB + (size_t)N * m;
  launch_lob_resid(lc, B, SB, R, Minv != nullptr ? W : nullptr,
                   part + LOB_GPART, N, m, s);
  if (Minv != nullptr)  // W was cleared by k_lob_resid
    launch_precond_dense(Minv, R, W, (int)N, m, lc, 0, s);
  else
    launch_precond_jacobi(L, R, W, n, d + 1, m, lc, 0, s);
  launch_lob_apply(lc, row_ptr, col_idx, vals, lam, W, SW, n, d, m, s);
  launch_lob_gram(lc, B, SB, part, part + LOB_GPART, out, N, m, s);
}

}  // extern "C"
