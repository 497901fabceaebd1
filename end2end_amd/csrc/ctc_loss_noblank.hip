// CTC without blank (ASG-style): the loss and its gradient, the sum-product twin of ctc_align.hip's is_ctc = 0 walk.
//
// Replaces pytorch_end2end/functions/ctc_without_blank.py:13-138 upstream (a numba lattice run on host copies, one Python
// thread per utterance).  Semantics restated exactly:
//   * extended target ext (L' cells): the target itself (space_idx = -1), else [sp] + target + [sp]; an empty target or
//     the target [sp] gives ext = [space_idx] -- with space_idx = -1 that is [-1], which numpy reads as column V-1 (Q10);
//   * from cell j a frame stays at j or moves to j+1 -- no blank, no skip, repeated labels allowed;
//   * start alpha[0] (and alpha[1] with the two spaces), end alpha[L'-1] (+ alpha[L'-2] with the two spaces);
//   * posterior per label: the cells that carry it summed in increasing j; gradient exp(lp) - posterior on frames
//     t < x_len, 0 beyond; an infeasible utterance gets loss +inf and NaN rows t < x_len.
// The upstream band limits only drop cells that cannot reach the end; the full lattice here gives the same numbers.
//
// Two launches per call.
//   noblank_rows_kernel     one wave per frame: the row's log-sum-exp (logits in: log-softmax fused; kept in the
//                           workspace) and the dense part of the gradient, grad[t, v] = scale * exp(lp[t, v]) (0 on
//                           padded frames).  Reads every row once; the lattice never reads a V-wide row again.
//   noblank_lattice_kernel  one 256-thread workgroup per utterance.  Wave 0 runs the serial recurrence out of LDS; waves
//                           1..3 gather the emissions p[t, ext[j]] of the NEXT block of kBlk frames into LDS (three
//                           buffers) and, in the backward sweep, finish the block before: for every distinct label u of the
//                           utterance (cells in label-sorted order) they fold the posterior and write
//                           grad[t, u] = scale * (exp(lp) - posterior) over the dense value.  One __syncthreads per block.
// Arithmetic.  f32 input: probability domain, f64 cells, every row divided by the power of two of its largest cell
// (exponents summed in an int), exp() once per cell.  Alpha rows are checkpointed every kBlk frames to the workspace;
// the backward sweep recomputes each block's rows into LDS from its checkpoint (bit-identical to the forward's) and
// runs beta over them.  An utterance the probability domain cannot settle -- a finite log-probability below -700, a
// row that under/overflows, a final total of 0 or non-finite although the lattice is structurally feasible -- is redone
// in the log domain by the same workgroup.  f64 input: the log domain throughout, upstream's log(1 + exp) and order.
// lattice_common.h holds what this file shares with ctc_loss_gram.hip: the row pass, the numeric helpers, the host call.
#include "common.h"
#include "lattice_common.h"

namespace e2e {
namespace {

constexpr int kNbBlk = 16;                   // frames per block = checkpoint interval (fewer from Smax 236 on: nb_block)
// LDS of one gfx950 workgroup, less the lattice kernel's static LDS: 288 bytes (f32; 272 f64), its own words and
// __syncthreads_or's; tests/test_noblank_cpu.py checks the built kernels against it
constexpr size_t kNbLdsMax = 160 * 1024 - 288;

struct NbParams {
  const void* x; int64_t sB, sT, sV;
  const int64_t* targets; int64_t tgt_stride;
  const int64_t* x_len; const int64_t* t_len;
  int B, T, V, Smax, space, logits, K, NB, Lmax;
  double gscale;
  void* losses; void* grads;
  const double* lse;                         // [B][T] row log-sum-exp (0 rows when x holds log-probabilities)
  double* ck;                                // [B][NB][Lmax] alpha checkpoint rows
  int* ckc;                                  // [B][NB] their power-of-two exponents
};

// order of a wave's LDS operations across steps (the LDS runs one wave's operations in order; this keeps the compiler's)
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

template <typename IO>
__global__ __launch_bounds__(256) void noblank_rows_kernel(NbParams p, double* lse_out) {
  loss_rows<IO>(p, lse_out);
}

// redo: [B] 0, or why the utterance was redone in the log domain (1 forward, 2 backward)
template <typename IO>
__global__ __launch_bounds__(kLatticeThreads) void noblank_lattice_kernel(NbParams p, int* redo) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Tmax = p.T, V = p.V, K = p.K, Lm = p.Lmax;
  // LDS: three emission buffers of K rows + one checkpoint row each, two blocks of alpha / posterior rows, two lattice rows
  double* pbuf = reinterpret_cast<double*>(smem);                    // [3][K + 1][Lm]
  double* ab = pbuf + 3 * (size_t)(K + 1) * Lm;                      // [2][K][Lm]
  double* rows = ab + 2 * (size_t)K * Lm;                            // [2][Lm]
  int* ext = reinterpret_cast<int*>(rows + 2 * (size_t)Lm);          // [Lm] label of every cell
  int* perm = ext + Lm;                                              // [Lm] cells in (label, j) order
  int* cb = perm + Lm;                                               // [2][K] exponents of the block rows
  __shared__ int s_flag, s_ckc[3], s_cend;

  IO* grads = reinterpret_cast<IO*>(p.grads) + (size_t)b * Tmax * V;
  typedef typename LossOf<IO>::type LT;
  LT* loss = reinterpret_cast<LT*>(p.losses) + b;
  const int64_t Tq = p.x_len[b], Sq = p.t_len[b];
  const bool bad_len = Tq < 1 || Tq > Tmax || Sq < 0 || Sq > p.Smax;
  const int T = bad_len ? 0 : (int)Tq, S = bad_len ? 0 : (int)Sq;
  const int64_t* tg = p.targets + (int64_t)b * p.tgt_stride;
  const int sp = p.space;
  if (tid == 0) redo[b] = 0;

  // ---- the extended target ----
  int bad = bad_len;
  for (int i = tid; i < S; i += kLatticeThreads) bad |= tg[i] < 0 || tg[i] >= V;
  bad = __syncthreads_or(bad);
  const bool single = S == 0 || (S == 1 && tg[0] == sp);
  const bool two = !single && sp >= 0;
  const int L = single ? 1 : two ? S + 2 : S;
  if (bad || L > Lm) {
    for (size_t i = tid; i < (size_t)Tmax * V; i += kLatticeThreads) grads[i] = (IO)NAN;
    if (tid == 0) *loss = (LT)NAN;
    return;
  }
  for (int i = tid; i < L; i += kLatticeThreads) {
    int lab;
    if (single) lab = sp < 0 ? V - 1 : sp;                           // ext = [space_idx]; [-1] is column V-1 (Q10)
    else if (two) lab = (i == 0 || i == L - 1) ? sp : (int)tg[i - 1];
    else lab = (int)tg[i];
    ext[i] = lab;
  }
  if (tid == 0) s_flag = 0;
  __syncthreads();
  for (int j = tid; j < L; j += kLatticeThreads) {                   // rank sort by (label, j)
    const int u = ext[j];
    int r = 0;
    for (int i = 0; i < L; i++) { const int w = ext[i]; r += (w < u) | ((w == u) & (i < j)); }
    perm[r] = j;
  }
  const bool feasible = two ? S <= T : L <= T;
  if (!feasible) {                                                   // no path: +inf, NaN rows (Q2's rule)
    for (size_t i = tid; i < (size_t)T * V; i += kLatticeThreads) grads[i] = (IO)NAN;
    if (tid == 0) *loss = (LT)INFINITY;
    return;
  }
  __syncthreads();

  const IO* x = reinterpret_cast<const IO*>(p.x) + (int64_t)b * p.sB;
  const double* lse = p.lse + (size_t)b * Tmax;
  double* ck = p.ck + (size_t)b * p.NB * Lm;
  int* ckc = p.ckc + (size_t)b * p.NB;
  const int NB = (T + K - 1) / K;
  const double scale = p.gscale;
  const bool logits = p.logits != 0;

  auto slot = [&](int n) __attribute__((always_inline)) { return pbuf + (size_t)(n % 3) * (K + 1) * Lm; };
  // emissions of block n into its slot (threads [first, first + count)): p = exp(lp) or lp itself in the log domain.
  // Sixteen loads in flight per thread.
  auto gather = [&](int n, bool logd, int first, int count, bool with_ck) __attribute__((always_inline)) {
    double* dst = slot(n);
    const int t0 = n * K, nk = min(K, T - t0), tot = nk * L;
    int low = 0;
    for (int base = tid - first; base < tot; base += 16 * count) {
      double v[16];
#pragma unroll
      for (int u = 0; u < 16; u++) {
        const int e = base + u * count;
        v[u] = 0.0;
        if (e < tot) {
          const int k = e / L, j = e - k * L;
          v[u] = (double)x[(int64_t)(t0 + k) * p.sT + (int64_t)ext[j] * p.sV] - (logits ? lse[t0 + k] : 0.0);
        }
      }
#pragma unroll
      for (int u = 0; u < 16; u++) {
        const int e = base + u * count;
        if (e < tot) {
          const int k = e / L, j = e - k * L;
          const double lp = v[u];
          low |= lp < kLowLp && lp > ninf();
          dst[(size_t)k * Lm + j] = logd ? lp : exp(lp);
        }
      }
    }
    if (with_ck) {
      for (int j = tid - first; j < L; j += count) dst[(size_t)K * Lm + j] = ck[(size_t)n * Lm + j];
      if (tid == first) s_ckc[n % 3] = ckc[n];
    }
    if (low) s_flag = 1;
  };

  bool logd = sizeof(IO) == 8;
  double zm = 0.0, logz = 0.0;
  int cend = 0;
  // grad[t, u] for the distinct labels u of block n (rows of alpha * beta in ab, emissions in the block's slot)
  auto finish = [&](int n, int first, int count) __attribute__((always_inline)) {
    const double* pb = slot(n);
    const double* A = ab + (size_t)(n & 1) * K * Lm;
    const int* e = cb + (n & 1) * K;
    const int t0 = n * K, nk = min(K, T - t0);
    for (int it = tid - first; it < nk * L; it += count) {
      const int k = it / L, q = it - k * L;
      const int j0 = perm[q], u = ext[j0];
      if (q > 0 && ext[perm[q - 1]] == u) continue;
      const double* a = A + (size_t)k * Lm;
      double acc = logd ? ninf() : 0.0;
      for (int i = q; i < L && ext[perm[i]] == u; i++) acc = logd ? lse2(acc, a[perm[i]]) : acc + a[perm[i]];
      const double post = logd ? exp(acc - logz) : ldexp(acc, e[k] - cend) / zm;
      const double pv = logd ? exp(pb[(size_t)k * Lm + j0]) : pb[(size_t)k * Lm + j0];
      grads[(size_t)(t0 + k) * V + u] = (IO)(scale * (pv - post));
    }
  };
  for (int pass = 0; pass < 2; pass++) {
    // ---- forward: alpha, checkpoint at the first frame of every block ----
    if (pass) __syncthreads();
    gather(0, logd, 0, kLatticeThreads, false);
    __syncthreads();
    int C = 0, m = 0, range_bad = 0;
    for (int n = 0; n < NB; n++) {
      if (wave == 0) {
        double* pb = slot(n);
        const int t0 = n * K, nk = min(K, T - t0);
        for (int k = 0; k < nk; k++) {
          const int t = t0 + k;
          const double* P = rows + (size_t)((t + 1) & 1) * Lm;
          double* Q = rows + (size_t)(t & 1) * Lm;
          const double* pr = pb + (size_t)k * Lm;
          int mx = 0;
          if (t == 0) {
            for (int j = lane; j < L; j += 64) {
              const double a = (j == 0 || (two && j == 1)) ? pr[j] : (logd ? ninf() : 0.0);
              Q[j] = a; mx = max(mx, expo(a));
            }
          } else if (logd) {
            for (int j = lane; j < L; j += 64) Q[j] = lse2(P[j], j > 0 ? P[j - 1] : ninf()) + pr[j];
          } else {
            C += m - 1023;
            const double sc = inv_pow2(m);
            for (int j = lane; j < L; j += 64) {
              const double a = (P[j] + (j > 0 ? P[j - 1] : 0.0)) * (pr[j] * sc);
              Q[j] = a; mx = max(mx, expo(a));
            }
          }
          wave_lds_sync();
          if (!logd) { m = wave_max_i(mx); range_bad |= expo_out_of_range(m); }
          if (k == 0) {                                  // checkpoint: to the workspace and into the slot's last row
            for (int j = lane; j < L; j += 64) { ck[(size_t)n * Lm + j] = Q[j]; pb[(size_t)K * Lm + j] = Q[j]; }
            if (lane == 0) { ckc[n] = C; s_ckc[n % 3] = C; }
          }
        }
      } else if (n + 1 < NB) {
        gather(n + 1, logd, 64, kLatticeThreads - 64, false);
      }
      __syncthreads();
    }
    const double* Q = rows + (size_t)((T - 1) & 1) * Lm;
    if (logd) {
      logz = two ? lse2(Q[L - 1], Q[L - 2]) : Q[L - 1];
    } else {
      if (tid == 0) s_cend = C;
      zm = two ? Q[L - 1] + Q[L - 2] : Q[L - 1];
      const int fail = prob_unsettled(range_bad, s_flag, zm);
      cend = s_cend;
      if (fail) {                                    // this utterance goes to the log domain
        if (tid == 0) redo[b] = 1;
        logd = true;
        continue;
      }
      logz = prob_log_z(zm, cend);
    }
    __syncthreads();                                 // (the last alpha row is read; beta takes its buffer)
    if (tid == 0) *loss = (LT)(-logz);
    if (logd && logz == ninf()) {                    // no path through the emissions: +inf, NaN rows
      for (size_t i = tid; i < (size_t)T * V; i += kLatticeThreads) grads[i] = (IO)NAN;
      return;
    }

    // ---- backward: per block (last first) wave 0 recomputes alpha from the checkpoint and runs beta over it; waves 1..3
    //      write the previous block's label columns and gather the next one ----
    int D = 0, f = 0, lost = 0;
    for (int n = NB - 1; n >= 0; n--) {
      if (wave == 0) {
        const double* pb = slot(n);
        double* A = ab + (size_t)(n & 1) * K * Lm;
        int* e = cb + (n & 1) * K;
        const int t0 = n * K, nk = min(K, T - t0);
        int C = s_ckc[n % 3], mx = 0;
        for (int j = lane; j < L; j += 64) { const double a = pb[(size_t)K * Lm + j]; A[j] = a; mx = max(mx, expo(a)); }
        if (lane == 0) e[0] = C;
        wave_lds_sync();
        int m = logd ? 0 : wave_max_i(mx);
        for (int k = 1; k < nk; k++) {
          const double* P = A + (size_t)(k - 1) * Lm;
          double* Q = A + (size_t)k * Lm;
          const double* pr = pb + (size_t)k * Lm;
          if (logd) {
            for (int j = lane; j < L; j += 64) Q[j] = lse2(P[j], j > 0 ? P[j - 1] : ninf()) + pr[j];
          } else {
            C += m - 1023;
            const double sc = inv_pow2(m);
            mx = 0;
            for (int j = lane; j < L; j += 64) {
              const double a = (P[j] + (j > 0 ? P[j - 1] : 0.0)) * (pr[j] * sc);
              Q[j] = a; mx = max(mx, expo(a));
            }
          }
          if (lane == 0) e[k] = C;
          wave_lds_sync();
          if (!logd) m = wave_max_i(mx);
        }
        // beta: s_t = G_{t+1}[j] + G_{t+1}[j+1] (scaled), G_t = s_t * p_t; the block's rows become alpha * s
        for (int k = nk - 1; k >= 0; k--) {
          const int t = t0 + k;
          const double* G = rows + (size_t)((t + 1) & 1) * Lm;
          double* H = rows + (size_t)(t & 1) * Lm;
          const double* pr = pb + (size_t)k * Lm;
          double* a = A + (size_t)k * Lm;
          int gx = 0;
          double mass = 0.0;
          if (t == T - 1) {
            for (int j = lane; j < L; j += 64) {
              const bool end = j == L - 1 || (two && j == L - 2);
              const double s = logd ? (end ? 0.0 : ninf()) : (end ? 1.0 : 0.0);
              a[j] = logd ? a[j] + s : a[j] * s;
              const double h = logd ? s + pr[j] : s * pr[j];
              H[j] = h; gx = max(gx, expo(h));
              mass += logd ? 0.0 : a[j];
            }
          } else if (logd) {
            for (int j = lane; j < L; j += 64) {
              const double s = lse2(G[j], j + 1 < L ? G[j + 1] : ninf());
              a[j] += s;
              H[j] = s + pr[j];
            }
          } else {
            D += f - 1023;
            const double sc = inv_pow2(f);
            for (int j = lane; j < L; j += 64) {
              const double s = (G[j] + (j + 1 < L ? G[j + 1] : 0.0)) * sc;
              const double as = a[j] * s, h = s * pr[j];
              a[j] = as; mass += as;
              H[j] = h; gx = max(gx, expo(h));
            }
          }
          const int ek = e[k] + D;
          if (lane == 0) e[k] = ek;
          wave_lds_sync();
          if (!logd) {
            f = wave_max_i(gx);
            lost |= expo_out_of_range(f);
            f = min(max(f, 1), 2045);
            mass = wave_sum(mass);
            lost |= !(fabs(ldexp(mass, ek - cend) / zm - 1.0) <= kMassTol);
          }
        }
      } else {
        if (n + 1 < NB) finish(n + 1, 64, kLatticeThreads - 64);
        // blocks NB-1 and NB-2 are still in their slots from the forward sweep
        if (n >= 1 && n - 1 < NB - 2) gather(n - 1, logd, 64, kLatticeThreads - 64, true);
      }
      __syncthreads();
    }
    finish(0, 0, kLatticeThreads);
    if (logd || !__syncthreads_or(lost)) break;
    if (tid == 0) redo[b] = 2;
    logd = true;
  }
}

// LDS of the lattice kernel for rows of Lmax cells and blocks of K frames
size_t nb_lds_bytes(int K, int Lmax) {
  return sizeof(double) * ((size_t)3 * (K + 1) * Lmax + (size_t)2 * K * Lmax + 2 * (size_t)Lmax) +
         sizeof(int) * (2 * (size_t)Lmax + 2 * (size_t)K) + 64;
}
int nb_lmax(int Smax) { return Smax + 2; }
int nb_block(int Lmax) {
  for (int K = kNbBlk; K >= 1; K--)
    if (nb_lds_bytes(K, Lmax) <= kNbLdsMax) return K;
  return 0;
}

LatticeLayout nb_layout(int B, int T, int Smax) {
  const int K = nb_block(nb_lmax(Smax));
  return lattice_layout(B, T, nb_lmax(Smax), K, K);                   // a checkpoint per block
}

}  // namespace
}  // namespace e2e

using namespace e2e;

extern "C" size_t e2e_ctc_noblank_workspace_bytes(int B, int T, int V, int Smax, int dtype) {
  (void)V; (void)dtype;
  if (B < 0 || T < 1 || Smax < 0) return 0;
  const LatticeLayout l = nb_layout(B, T, Smax);
  return l.K ? l.total + 256 : 0;
}

extern "C" int e2e_ctc_noblank_fwd_bwd(const void* x, int dtype, int input_is_logprobs, int64_t sB, int64_t sT, int64_t sV,
                                       const int64_t* targets, int64_t tgt_stride, const int64_t* x_len,
                                       const int64_t* t_len, int B, int T, int V, int Smax, int space_idx, void* losses,
                                       void* grads, void* workspace, size_t workspace_bytes, void* stream,
                                       const e2e_ctc_loss_opts* opts) {
  LossArgs a{x, dtype, input_is_logprobs ? 1 : 0, sB, sT, sV, targets, tgt_stride, x_len, t_len,
             B, T, V, Smax, 0, losses, grads, workspace, workspace_bytes, (hipStream_t)stream};
  int rc = lattice_check_args(a, opts);
  if (rc != E2E_OK) return rc;
  if (space_idx != -1 && (space_idx < 0 || space_idx >= V)) { set_error("space_idx=%d is neither -1 nor in [0,%d)", space_idx, V); return E2E_ERR_ARG; }
  const LatticeLayout l = nb_layout(B, T, Smax);
  if (l.K == 0) { set_error("CTC without blank: Smax=%d needs more than %zu B of LDS", Smax, kNbLdsMax); return E2E_ERR_UNSUPPORTED; }
  rc = lattice_workspace(a, l);
  if (rc != E2E_OK || B == 0) return rc;
  NbParams p;
  lattice_params(p, a, l);
  p.space = space_idx; p.Lmax = l.cells;
  static const LatticeKernels<NbParams, int*> kernels = {
      noblank_rows_kernel<float>, noblank_rows_kernel<double>, "noblank_rows_kernel launch",
      noblank_lattice_kernel<float>, noblank_lattice_kernel<double>, "noblank_lattice_kernel launch"};
  return lattice_launch(a, kernels, p, nb_lds_bytes(l.K, l.cells), reinterpret_cast<int*>(aligned_256(workspace) + l.redo));
}

// Diagnostics: after an e2e_ctc_noblank_fwd_bwd call with this workspace, why each utterance was redone in the log domain
// (0 not redone, f64 input, or no lattice run; 1 the forward could not settle it, 2 the backward lost mass or range).
// Synchronises.
extern "C" int e2e_debug_noblank_redo_flags(const void* workspace, int B, int T, int Smax, int* flags_host) {
  if (!workspace || !flags_host || B < 1 || T < 1 || Smax < 0) { set_error("bad arguments"); return E2E_ERR_ARG; }
  return lattice_redo_flags(workspace, nb_layout(B, T, Smax), B, flags_host);
}
