// Gram-CTC (Liu et al., ICML 2017): the loss and its gradient.  Upstream ships the class and an empty engine
// (src/losses/gram_ctc_loss.cpp:30-37); the definition here is the one of include/e2e_ctc.h and DESIGN.md 4.6:
//   * column 0 is the blank; columns 1..R-1 are the unigrams of the base labels 1..R-1; columns R..V-1 are grams, each
//     a sequence of 1..8 base labels, found through a table of sorted keys (the sequence read as a number in radix R);
//   * a path's labelling: collapse runs of one column, drop blanks, concatenate the grams' base sequences;
//   * the loss is -log of the total probability of the paths whose labelling is the target.
// Lattice over the target's boundaries j = 0..S: a blank state at every boundary, a gram state (j, k) wherever
// y[j-k..j-1] is a gram (k <= max_order).  blank(j) takes from itself and every gram state ending at j; gram(j, k) from
// itself, blank(j-k) and every gram state ending at j-k except one of the same column.  Start blank(0) and gram(k, k);
// end blank(S) and every gram(S, k).  With unigrams only this is CTC with blank 0.
//
// Two launches per call.
//   gram_rows_kernel     one wave per frame: the row's log-sum-exp (logits in: log-softmax fused; kept in the workspace)
//                        and the dense part of the gradient, grad[t, v] = scale * exp(lp[t, v]) (0 on padded frames):
//                        lattice_common.h, shared with ctc_loss_noblank.hip.
//   gram_lattice_kernel  one 256-thread workgroup per utterance.  Prologue: every cell (j, k) of the target is matched
//                        against the gram table (binary search), repeated grams are marked, and the gram cells are sorted
//                        by (column, cell).  Rows of (S+1) * (max_order+1) cells, one boundary per thread, all four waves
//                        on the serial recurrence with one barrier per frame; each block of K frames has its emissions
//                        gathered into LDS first.  The backward sweep writes one posterior per column present.
// Arithmetic: ctc_loss_noblank.hip's, its helpers and the host call in lattice_common.h.  f32 input: probability domain, f64 cells, every row divided by the power of two of
// its largest cell (a workgroup-wide max, carried to the next frame through LDS), alpha rows checkpointed every kCk frames;
// the backward recomputes each block's rows from its checkpoint (bit-identical to the forward's) and runs beta over them.
// An utterance the probability domain cannot settle -- a finite log-probability below -700, a row that under/overflows, a
// total of 0 or non-finite, a frame whose posteriors do not sum to 1 -- is redone by the same workgroup in the log domain,
// which f64 input always uses.
#include "common.h"
#include "lattice_common.h"

namespace e2e {
namespace {

constexpr int kGcWaves = kLatticeThreads / 64;
constexpr int kCk = 16;                      // checkpoint interval (frames); the LDS block K divides it
constexpr int kGcMaxOrder = 8;
constexpr size_t kGcLdsMax = 160 * 1024 - 256;   // LDS of one gfx950 workgroup, less the kernel's own words

struct GcParams {
  const void* x; int64_t sB, sT, sV;
  const int64_t* targets; int64_t tgt_stride;
  const int64_t* x_len; const int64_t* t_len;
  const int64_t* keys; const int* cols;      // gram table: sorted keys, their columns
  int B, T, V, Smax, R, M, n_grams, logits, K, NB;
  double gscale;
  void* losses; void* grads;
  const double* lse;                         // [B][T] row log-sum-exp (0 rows when x holds log-probabilities)
  double* ck;                                // [B][NB][NC] alpha checkpoint rows, NC = (Smax + 1) * (M + 1)
  int* ckc;                                  // [B][NB] their power-of-two exponents
  int* redo;                                 // [B] 0, or why the utterance was redone in the log domain (1 forward, 2 backward)
};

template <typename IO>
__global__ __launch_bounds__(256) void gram_rows_kernel(GcParams p, double* lse_out) {
  loss_rows<IO>(p, lse_out);
}

// cell (j, k) of a row is j * M1 + k: k = 0 the blank of boundary j, k >= 1 the gram y[j-k..j-1] (if it is one).
// flag: bit 0 the cell is a state, bit 1 (gram cells) the gram state (j-k, k) exists and has the same column.
template <typename IO>
__global__ __launch_bounds__(kLatticeThreads) void gram_lattice_kernel(GcParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Tmax = p.T, V = p.V, K = p.K, M = p.M, M1 = p.M + 1;
  const int NC = (p.Smax + 1) * M1;
  double* pbuf = reinterpret_cast<double*>(smem);                    // [K][NC] emissions of the block
  double* ab = pbuf + (size_t)K * NC;                                // [K][NC] alpha rows of the block, then alpha * beta
  double* rows = ab + (size_t)K * NC;                                // [2][NC] forward alpha / beta rows
  double* pre = rows + 2 * (size_t)NC;                               // [2][NC] alpha rows ahead of a block (backward)
  double* wsum = pre + 2 * (size_t)NC;                               // [K][4] per-wave mass of every frame of the block
  int* col = reinterpret_cast<int*>(wsum + (size_t)K * kGcWaves);    // [NC] column of every cell (-1: no state)
  int* flag = col + NC;                                              // [NC]
  int* perm = flag + NC;                                             // [NC] gram cells in (column, cell) order
  int* tg = perm + NC;                                               // [Smax + 1] the target
  int* cb = tg + p.Smax + 1;                                         // [K] exponents of the block rows
  int* wm = cb + K;                                                  // [2][4] per-wave largest exponent of an alpha row
  int* wmb = wm + 2 * kGcWaves;                                      // [2][4] the same for beta rows
  __shared__ int s_flag, s_lost, s_ng;

  IO* grads = reinterpret_cast<IO*>(p.grads) + (size_t)b * Tmax * V;
  typedef typename LossOf<IO>::type LT;
  LT* loss = reinterpret_cast<LT*>(p.losses) + b;
  const int64_t Tq = p.x_len[b], Sq = p.t_len[b];
  const bool bad_len = Tq < 1 || Tq > Tmax || Sq < 0 || Sq > p.Smax;
  const int T = bad_len ? 0 : (int)Tq, S = bad_len ? 0 : (int)Sq;
  const int64_t* tgg = p.targets + (int64_t)b * p.tgt_stride;
  if (tid == 0) p.redo[b] = 0;

  // ---- prologue: the target, the states, the column order ----
  int bad = bad_len;
  for (int i = tid; i < S; i += kLatticeThreads) {
    const int64_t y = tgg[i];
    bad |= y < 1 || y >= p.R;
    tg[i] = (int)y;
  }
  bad = __syncthreads_or(bad);
  if (bad) {
    for (size_t i = tid; i < (size_t)Tmax * V; i += kLatticeThreads) grads[i] = (IO)NAN;
    if (tid == 0) *loss = (LT)NAN;
    return;
  }
  const int NCu = (S + 1) * M1;
  for (int c = tid; c < NCu; c += kLatticeThreads) {
    const int j = c / M1, k = c - j * M1;
    int u = k == 0 ? 0 : -1;
    if (k > 0 && j >= k) {
      int64_t key = 0;
      for (int i = j - k; i < j; i++) key = key * p.R + tg[i];
      int lo = 0, hi = p.n_grams;                  // first key >= key
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (p.keys[mid] < key) lo = mid + 1; else hi = mid;
      }
      if (lo < p.n_grams && p.keys[lo] == key) {
        const int c = p.cols[lo];
        if (c >= 1 && c < V) u = c;                 // (a column outside the logits is no state)
      }
    }
    col[c] = u;
  }
  if (tid == 0) { s_flag = 0; s_lost = 0; s_ng = 0; }
  __syncthreads();
  int ng = 0;
  for (int c = tid; c < NCu; c += kLatticeThreads) {
    const int j = c / M1, k = c - j * M1, u = col[c];
    int f = u >= 0;
    if (k > 0 && u >= 0 && j >= 2 * k && col[c - k * M1] == u) f |= 2;
    flag[c] = f;
    if (k > 0 && u >= 1) {                          // rank among the gram cells by (column, cell)
      int r = 0;
      for (int i = 0; i < NCu; i++) { const int w = col[i]; r += (i % M1 != 0) & (w >= 1) & ((w < u) | ((w == u) & (i < c))); }
      perm[r] = c;
      ng++;
    }
  }
  if (ng) atomicAdd(&s_ng, ng);
  __syncthreads();
  const int NG = s_ng;

  const IO* x = reinterpret_cast<const IO*>(p.x) + (int64_t)b * p.sB;
  const double* lse = p.lse + (size_t)b * Tmax;
  double* ck = p.ck + (size_t)b * p.NB * NC;
  int* ckc = p.ckc + (size_t)b * p.NB;
  const double scale = p.gscale;
  const bool logits = p.logits != 0;
  bool logd = sizeof(IO) == 8;
  const double zero = 0.0;

  // emissions of frames [t0, t0 + nk) into pbuf: p = exp(lp), or lp itself in the log domain; 16 loads in flight per thread
  auto gather = [&](int t0, int nk) __attribute__((always_inline)) {
    const int tot = nk * NCu;
    int low = 0;
    for (int base = tid; base < tot; base += 16 * kLatticeThreads) {
      double v[16];
#pragma unroll
      for (int u = 0; u < 16; u++) {
        const int e = base + u * kLatticeThreads;
        v[u] = ninf();
        if (e < tot) {
          const int k = e / NCu, c = e - k * NCu, cu = col[c];
          if (cu >= 0) v[u] = (double)x[(int64_t)(t0 + k) * p.sT + (int64_t)cu * p.sV] - (logits ? lse[t0 + k] : 0.0);
        }
      }
#pragma unroll
      for (int u = 0; u < 16; u++) {
        const int e = base + u * kLatticeThreads;
        if (e < tot) {
          const int k = e / NCu, c = e - k * NCu;
          const double lp = v[u];
          low |= lp < kLowLp && lp > ninf();
          pbuf[(size_t)k * NC + c] = logd ? lp : exp(lp);
        }
      }
    }
    if (low) s_flag = 1;
  };
  // alpha row Q of a frame from the row P before it (first: the frame 0 row), emissions pr, row scale sc; returns the
  // thread's largest exponent
  auto alpha_row = [&](const double* P, double* Q, const double* pr, double sc, bool first) __attribute__((always_inline)) {
    int mx = 0;
    for (int j = tid; j <= S; j += kLatticeThreads) {
      const double* Pj = P + j * M1;
      for (int k = 0; k <= M; k++) {
        const int c = j * M1 + k, f = flag[c];
        double a;
        if (!(f & 1)) {
          a = logd ? ninf() : zero;
        } else if (first) {
          a = (k == 0 ? j == 0 : j == k) ? pr[c] : (logd ? ninf() : zero);
        } else if (k == 0) {
          double s = Pj[0];
          for (int i = 1; i <= M; i++) s = logd ? lse2(s, Pj[i]) : s + Pj[i];
          a = logd ? s + pr[c] : s * (pr[c] * sc);
        } else {
          const double* Pb = P + (j - k) * M1;
          const int skip = (f & 2) ? k : 0;
          double s = logd ? lse2(Pj[k], Pb[0]) : Pj[k] + Pb[0];
          for (int i = 1; i <= M; i++)
            if (i != skip) s = logd ? lse2(s, Pb[i]) : s + Pb[i];
          a = logd ? s + pr[c] : s * (pr[c] * sc);
        }
        Q[c] = a;
        mx = max(mx, expo(a));
      }
    }
    return mx;
  };
  // a row's largest exponent through LDS: each wave's max into wm[par], read after the barrier that follows
  auto put_max = [&](int mx, int par, int* w) __attribute__((always_inline)) {
    mx = wave_max_i(mx);
    if (lane == 0) w[par * kGcWaves + wave] = mx;
  };
  auto get_max = [&](int par, const int* wv) __attribute__((always_inline)) {
    const int* w = wv + par * kGcWaves;
    return max(max(w[0], w[1]), max(w[2], w[3]));
  };

  double zm = 0.0, logz = 0.0;
  int cend = 0;
  // grad[t, u] for the columns u of the frames [t0, t0 + nk) (alpha * beta in ab, emissions in pbuf); the frames' mass
  auto finish = [&](int t0, int nk) __attribute__((always_inline)) {
    for (int it = tid; it < nk * NG; it += kLatticeThreads) {
      const int k = it / NG, q = it - k * NG;
      const int c0 = perm[q], u = col[c0];
      if (q > 0 && col[perm[q - 1]] == u) continue;
      const double* a = ab + (size_t)k * NC;
      double acc = logd ? ninf() : 0.0;
      for (int i = q; i < NG && col[perm[i]] == u; i++) acc = logd ? lse2(acc, a[perm[i]]) : acc + a[perm[i]];
      const double post = logd ? exp(acc - logz) : ldexp(acc, cb[k] - cend) / zm;
      const double pv = logd ? exp(pbuf[(size_t)k * NC + c0]) : pbuf[(size_t)k * NC + c0];
      grads[(size_t)(t0 + k) * V + u] = (IO)(scale * (pv - post));
    }
    for (int k = wave; k < nk; k += kGcWaves) {      // the blank column: one wave per frame
      const double* a = ab + (size_t)k * NC;
      double acc = logd ? ninf() : 0.0;
      for (int j = lane; j <= S; j += 64) acc = logd ? lse2(acc, a[j * M1]) : acc + a[j * M1];
      acc = logd ? wave_lse(acc) : wave_sum(acc);
      if (lane == 0) {
        const double post = logd ? exp(acc - logz) : ldexp(acc, cb[k] - cend) / zm;
        const double pv = logd ? exp(pbuf[(size_t)k * NC]) : pbuf[(size_t)k * NC];
        grads[(size_t)(t0 + k) * V] = (IO)(scale * (pv - post));
        if (!logd) {
          const double* w = wsum + (size_t)k * kGcWaves;
          const double mass = (w[0] + w[1]) + (w[2] + w[3]);
          if (!(fabs(ldexp(mass, cb[k] - cend) / zm - 1.0) <= kMassTol)) s_lost = 1;
        }
      }
    }
  };

  const int NBk = (T + K - 1) / K;
  for (int pass = 0; pass < 2; pass++) {
    // ---- forward: alpha, checkpoint at every kCk-th frame ----
    if (pass) __syncthreads();
    int C = 0, range_bad = 0;
    for (int n = 0; n < NBk; n++) {
      const int t0 = n * K, nk = min(K, T - t0);
      gather(t0, nk);
      __syncthreads();
      for (int k = 0; k < nk; k++) {
        const int t = t0 + k;
        double sc = 1.0;
        if (t > 0 && !logd) {
          const int m = get_max((t - 1) & 1, wm);
          range_bad |= expo_out_of_range(m);
          C += m - 1023;
          sc = inv_pow2(m);
        }
        double* Q = rows + (size_t)(t & 1) * NC;
        const int mx = alpha_row(rows + (size_t)((t + 1) & 1) * NC, Q, pbuf + (size_t)k * NC, sc, t == 0);
        if (!logd) put_max(mx, t & 1, wm);
        if (t % kCk == 0) {                          // (each thread stores the cells it wrote: no barrier needed)
          for (int j = tid; j <= S; j += kLatticeThreads)
            for (int k2 = 0; k2 <= M; k2++) ck[(size_t)(t / kCk) * NC + j * M1 + k2] = Q[j * M1 + k2];
          if (tid == 0) ckc[t / kCk] = C;
        }
        __syncthreads();
      }
    }
    const double* Q = rows + (size_t)((T - 1) & 1) * NC + (size_t)S * M1;
    double z = Q[0];
    for (int i = 1; i <= M; i++) z = logd ? lse2(z, Q[i]) : z + Q[i];
    if (logd) {
      logz = z;
    } else {
      const int m = get_max((T - 1) & 1, wm);
      range_bad |= expo_out_of_range(m);
      zm = z;
      cend = C;
      if (prob_unsettled(range_bad, s_flag, zm)) {                                    // this utterance goes to the log domain
        if (tid == 0) p.redo[b] = 1;
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

    // ---- backward: per block of K frames (last first) alpha is recomputed from its checkpoint (through the frames
    //      before the block inside the checkpoint interval), beta runs over it, the block's columns are written ----
    int D = 0, f = 0, lost = 0;
    for (int n = NBk - 1; n >= 0; n--) {
      const int t0 = n * K, nk = min(K, T - t0), ts = t0 / kCk * kCk;
      // the checkpoint row of frame ts: into ab row 0 when it is the block's first frame, else into pre
      double* R0 = ts == t0 ? ab : pre;
      int C = ckc[ts / kCk], mx = 0;
      for (int c = tid; c < NCu; c += kLatticeThreads) {
        const double a = ck[(size_t)(ts / kCk) * NC + c];
        R0[c] = a; mx = max(mx, expo(a));
      }
      if (!logd) put_max(mx, ts & 1, wm);
      if (tid == 0) cb[0] = C;
      __syncthreads();
      const double* P = R0;
      for (int c0 = ts; c0 < t0 + nk; c0 += K) {      // chunks of K frames: those ahead of the block, then the block
        gather(c0, min(K, T - c0));
        __syncthreads();
        for (int t = max(c0, ts + 1); t < min(c0 + K, t0 + nk); t++) {
          double sc = 1.0;
          if (!logd) {
            const int m = get_max((t - 1) & 1, wm);
            C += m - 1023;
            sc = inv_pow2(m);
          }
          double* Qr = t >= t0 ? ab + (size_t)(t - t0) * NC : pre + (size_t)((t - ts) & 1) * NC;
          const int m2 = alpha_row(P, Qr, pbuf + (size_t)(t - c0) * NC, sc, false);
          if (!logd) put_max(m2, t & 1, wm);
          if (t >= t0 && tid == 0) cb[t - t0] = C;
          __syncthreads();
          P = Qr;
        }
      }
      // beta: s_t = sum of the successors' G_{t+1} (scaled), G_t = s_t * p_t; the block's rows become alpha * s
      for (int k = nk - 1; k >= 0; k--) {
        const int t = t0 + k;
        const double* G = rows + (size_t)((t + 1) & 1) * NC;
        double* H = rows + (size_t)(t & 1) * NC;
        const double* pr = pbuf + (size_t)k * NC;
        double* a = ab + (size_t)k * NC;
        double sc = 1.0;
        if (t < T - 1 && !logd) {
          f = get_max((t + 1) & 1, wmb);
          lost |= expo_out_of_range(f);
          f = min(max(f, 1), 2045);
          D += f - 1023;
          sc = inv_pow2(f);
        }
        int gx = 0;
        double mass = 0.0;
        for (int j = tid; j <= S; j += kLatticeThreads) {
          for (int k2 = 0; k2 <= M; k2++) {
            const int c = j * M1 + k2;
            double s;
            if (!(flag[c] & 1)) {
              s = logd ? ninf() : zero;
            } else if (t == T - 1) {
              s = j == S ? (logd ? 0.0 : 1.0) : (logd ? ninf() : zero);
            } else {
              // successors: itself, the blank of j (from a gram), and every gram (j+i, i) except a repeat of this one
              int skip = 0;
              if (k2 > 0 && j + k2 <= S && (flag[c + k2 * M1] & 2)) skip = k2;
              double acc = G[c];
              if (k2 > 0) acc = logd ? lse2(acc, G[j * M1]) : acc + G[j * M1];
              for (int i = 1; i <= M && j + i <= S; i++)
                if (i != skip) acc = logd ? lse2(acc, G[(j + i) * M1 + i]) : acc + G[(j + i) * M1 + i];
              s = logd ? acc : acc * sc;
            }
            const double as = logd ? a[c] + s : a[c] * s;
            const double h = logd ? s + pr[c] : s * pr[c];
            a[c] = as;
            H[c] = h;
            mass += logd ? 0.0 : as;
            gx = max(gx, expo(h));
          }
        }
        if (!logd) {
          put_max(gx, t & 1, wmb);
          mass = wave_sum(mass);
          if (lane == 0) wsum[(size_t)k * kGcWaves + wave] = mass;
        }
        if (tid == 0) cb[k] += D;
        __syncthreads();
      }
      finish(t0, nk);
      __syncthreads();
    }
    if (logd || !__syncthreads_or(lost || s_lost)) break;
    if (tid == 0) p.redo[b] = 2;
    logd = true;
  }
}

// LDS of the lattice kernel for rows of NC cells, targets of up to Smax labels and blocks of K frames
size_t gc_lds_bytes(int K, int NC, int Smax) {
  return sizeof(double) * ((size_t)2 * K * NC + 4 * (size_t)NC + (size_t)K * kGcWaves) +
         sizeof(int) * (3 * (size_t)NC + (size_t)Smax + 1 + K + 4 * kGcWaves) + 64;
}
// the LDS block: the largest divisor of kCk that fits (0: none does)
int gc_block(int NC, int Smax) {
  for (int K = kCk; K >= 1; K /= 2)
    if (gc_lds_bytes(K, NC, Smax) <= kGcLdsMax) return K;
  return 0;
}

LatticeLayout gc_layout(int B, int T, int Smax, int max_order) {
  if ((int64_t)(Smax + 1) * (max_order + 1) > (1 << 20)) return LatticeLayout{};
  const int NC = (Smax + 1) * (max_order + 1);
  return lattice_layout(B, T, NC, gc_block(NC, Smax), kCk);
}

}  // namespace
}  // namespace e2e

using namespace e2e;

extern "C" size_t e2e_gram_ctc_workspace_bytes(int B, int T, int V, int Smax, int max_order, int dtype) {
  (void)V; (void)dtype;
  if (B < 0 || T < 1 || Smax < 0 || max_order < 1 || max_order > kGcMaxOrder) return 0;
  const LatticeLayout l = gc_layout(B, T, Smax, max_order);
  return l.K ? l.total + 256 : 0;
}

extern "C" int e2e_gram_ctc_fwd_bwd(const void* x, int dtype, int input_is_logprobs, int64_t sB, int64_t sT, int64_t sV,
                                    const int64_t* targets, int64_t tgt_stride, const int64_t* x_len,
                                    const int64_t* t_len, int B, int T, int V, int Smax, const int64_t* keys,
                                    const int32_t* cols, int n_grams, int radix, int max_order, void* losses,
                                    void* grads, void* workspace, size_t workspace_bytes, void* stream,
                                    const e2e_ctc_loss_opts* opts) {
  LossArgs a{x, dtype, input_is_logprobs ? 1 : 0, sB, sT, sV, targets, tgt_stride, x_len, t_len,
             B, T, V, Smax, 0, losses, grads, workspace, workspace_bytes, (hipStream_t)stream};
  int rc = lattice_check_args(a, opts);
  if (rc != E2E_OK) return rc;
  if (radix < 1 || radix > V) { set_error("radix=%d is not in [1, V=%d]", radix, V); return E2E_ERR_ARG; }
  if (max_order < 1 || max_order > kGcMaxOrder) { set_error("max_order=%d is not in [1, %d]", max_order, kGcMaxOrder); return E2E_ERR_ARG; }
  {
    int64_t r = 1;
    for (int i = 0; i < max_order; i++) {
      if (r > INT64_MAX / radix) { set_error("radix=%d ** max_order=%d overflows int64", radix, max_order); return E2E_ERR_ARG; }
      r *= radix;
    }
  }
  if (n_grams < 0 || (n_grams > 0 && (!keys || !cols))) { set_error("bad gram table: n_grams=%d", n_grams); return E2E_ERR_ARG; }
  const LatticeLayout l = gc_layout(B, T, Smax, max_order);
  if (l.K == 0) {
    set_error("Gram-CTC: Smax=%d at max_order=%d needs more than %zu B of LDS", Smax, max_order, kGcLdsMax);
    return E2E_ERR_UNSUPPORTED;
  }
  rc = lattice_workspace(a, l);
  if (rc != E2E_OK || B == 0) return rc;
  GcParams p;
  lattice_params(p, a, l);
  p.keys = keys; p.cols = cols; p.R = radix; p.M = max_order; p.n_grams = n_grams;
  p.redo = reinterpret_cast<int*>(aligned_256(workspace) + l.redo);
  static const LatticeKernels<GcParams> kernels = {
      gram_rows_kernel<float>, gram_rows_kernel<double>, "gram_rows_kernel launch",
      gram_lattice_kernel<float>, gram_lattice_kernel<double>, "gram_lattice_kernel launch"};
  return lattice_launch(a, kernels, p, gc_lds_bytes(l.K, l.cells, Smax));
}

// Diagnostics: after an e2e_gram_ctc_fwd_bwd call with this workspace, why each utterance was redone in the log domain
// (0 not redone or f64 input, 1 the forward could not settle it, 2 the backward lost mass or range).  Synchronises.
extern "C" int e2e_debug_gram_redo_flags(const void* workspace, int B, int T, int Smax, int max_order, int* flags_host) {
  if (!workspace || !flags_host || B < 1 || T < 1 || Smax < 0 || max_order < 1 || max_order > kGcMaxOrder) {
    set_error("bad arguments"); return E2E_ERR_ARG;
  }
  return lattice_redo_flags(workspace, gc_layout(B, T, Smax, max_order), B, flags_host);
}
