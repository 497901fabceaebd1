// ASG, the Auto Segmentation Criterion (Collobert et al. 2016, arXiv:1609.03193): the loss with learned transitions, both of
// its gradients, and the best path.  The definition is include/e2e_ctc.h's; upstream names ASG (ASGEncoder, the "ASG-style"
// lattice of CTC without blank) and implements none of it.
//   x (B,T,V) emissions, unnormalised; A (V,V) transitions, A[j,i] = score of label j at frame t after label i at t-1.
//   loss_b = FCC_b - FAL_b: log-sum-exp of the path score over all V^n label paths, minus the same over the alignments of
//   the target (the blank-free lattice of ctc_loss_noblank.hip with a multiplier on each of a cell's two arcs).
//
// Three kernels, one 256-thread workgroup per utterance each, all cells f64 for f32 and f64 inputs alike.
//   asg_fcc_kernel      the dense recurrence.  State: log alpha_t[v].  A step shifts by the row maximum m and leaves the log
//                       domain for the V x V product only: alpha_t[j] = x_t[j] + m + Amax + log(sum_i E[j,i] e^(alpha[i]-m))
//                       with E = exp(A - Amax) in LDS ([VP][VP + 1], VP = 32 / 64 / 128 the padded alphabet).  A term that
//                       underflows is below e^-700 of the row's largest: no redo route is needed.  The V^2 products of a
//                       frame are spread over the workgroup: thread (j, part) sums a slice of row j, V threads add the
//                       parts in a fixed order and take the log.  log alpha of every frame goes to the workspace.  The
//                       backward sweep runs beta the same way with thread (part, i) on a slice of column i; the product
//                       E[j,i] e^(w[j]-mb) it forms is also the pair posterior's, up to the column factor
//                       e^(alpha_{t-1}[i] + Amax + mb - FCC), and each thread keeps the sums of its VP^2/256 pairs in
//                       registers over the whole utterance.  Writes grads = scale * P_fcc and the pair sums (f64, workspace).
//   asg_fal_kernel      the target lattice in the log domain, two cells per thread, one barrier per frame; alpha rows in the
//                       workspace.  Subtracts the cell posteriors from grads (cells of one label summed in cell order, as
//                       the blank-free kernel does), keeps per-cell stay / advance sums in registers, and writes
//                       tgrads[j,i] = scale * (pair sum - sum over the cells that put mass on A[j,i], in cell order).
//                       Writes the losses, and the NaN / +inf slabs of utterances without a lattice.
//   asg_viterbi_kernel  the max-plus twin of the forward sweep, f64 in the order the header states, one-byte back-pointers
//                       in the workspace; thread 0 walks them back and merges repeats.
// Nothing is accumulated by atomics: every sum has one owner and a fixed order, so results are bit-identical call to call.
#include "common.h"
#include "lattice_common.h"

namespace e2e {
namespace {

constexpr int kAsgMaxV = 128;                // alphabet columns: E = exp(A) must fit in one workgroup's LDS beside the vectors
constexpr int kAsgMaxS = 512;                // target labels: the FAL kernel's rows are static LDS arrays
constexpr double kAsgExpCap = 700.0;         // a column factor beyond e^700 multiplies products that are below e^-700

struct AsgParams {
  const void* x; int64_t sB, sT, sV;
  const void* trans;                         // (V,V) contiguous, the I/O dtype
  const int64_t* targets; int64_t tgt_stride;
  const int64_t* x_len; const int64_t* t_len;
  int B, T, V, Smax, Sp;                     // Sp = max(Smax, 1): cells per FAL row in the workspace
  double gscale;
  void* losses; void* grads; void* tgrads;
  double* la;                                // [B][T][V] log alpha of the dense recurrence
  double* gf;                                // [B][V][V] its pair posteriors summed over the frames
  double* fcc;                               // [B]
  double* fa;                                // [B][T][Sp] log alpha of the target lattice
};

struct AsgVitParams {
  const void* x; int64_t sB, sT, sV;
  const void* trans;
  const int64_t* x_len;
  int B, T, V;
  int64_t* path; int64_t pad; double* scores; int64_t* collapsed; int64_t* lengths;
  unsigned char* bp;                         // [B][T][V] back-pointers
};

__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// LDS of the dense kernels: the matrix [VP][VP + 1], the state vector [VP], the partial sums [256], the waves' maxima [4]
constexpr size_t asg_dense_lds(int VP) { return sizeof(double) * ((size_t)VP * (VP + 1) + VP + kLatticeThreads + 8); }

template <typename IO, int VP>
__global__ __launch_bounds__(kLatticeThreads) void asg_fcc_kernel(AsgParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int NPT = VP * VP / kLatticeThreads;       // pairs per thread; also the slice of a row / column a thread sums
  constexpr int PARTS = kLatticeThreads / VP;          // threads per row / column
  constexpr int PITCH = VP + 1;
  double* eA = reinterpret_cast<double*>(smem);        // [VP][PITCH] exp(A - Amax), 0 outside V x V
  double* vec = eA + (size_t)VP * PITCH;               // [VP]
  double* part = vec + VP;                             // [256]
  double* red = part + kLatticeThreads;                // [4]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = p.V, Tmax = p.T;
  const int64_t Tq = p.x_len[b];
  if (Tq < 1 || Tq > Tmax) return;                     // (the FAL kernel writes this utterance's NaN slabs)
  const int n = (int)Tq;
  const IO* x = reinterpret_cast<const IO*>(p.x) + (int64_t)b * p.sB;
  const IO* At = reinterpret_cast<const IO*>(p.trans);
  double* la = p.la + (size_t)b * Tmax * V;
  IO* grads = reinterpret_cast<IO*>(p.grads) + (size_t)b * Tmax * V;

  // the workgroup's maximum of one value per thread (a barrier: every thread calls it)
  auto block_max = [&](double v) __attribute__((always_inline)) {
    v = wave_max_d(v);
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  };

  double amax = ninf();
  for (int e = tid; e < V * V; e += kLatticeThreads) amax = fmax(amax, (double)At[e]);
  amax = block_max(amax);
  for (int e = tid; e < VP * VP; e += kLatticeThreads) {
    const int j = e / VP, i = e % VP;
    eA[(size_t)j * PITCH + i] = (j < V && i < V) ? exp((double)At[j * V + i] - amax) : 0.0;
  }
  for (size_t i = (size_t)n * V + tid; i < (size_t)Tmax * V; i += kLatticeThreads) grads[i] = (IO)0;   // padded frames
  __syncthreads();                                     // (the maxima are read; the next block_max takes their words)

  // ---- forward: thread (rj, rp) sums the slice rp of row rj ----
  const int rj = tid & (VP - 1), rp = tid / VP;
  double cur = ninf();                                 // log alpha_t[tid]
  if (tid < V) { cur = (double)x[(int64_t)tid * p.sV]; la[tid] = cur; }
  for (int t = 1; t < n; t++) {
    const double xt = tid < V ? (double)x[(int64_t)t * p.sT + (int64_t)tid * p.sV] : 0.0;
    double m = block_max(cur);
    if (!(m > ninf())) m = 0.0;
    if (tid < VP) vec[tid] = tid < V ? exp(cur - m) : 0.0;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < NPT; u++) { const int i = rp * NPT + u; s += eA[(size_t)rj * PITCH + i] * vec[i]; }
    part[tid] = s;
    __syncthreads();
    if (tid < V) {
      s = 0.0;
#pragma unroll
      for (int q = 0; q < PARTS; q++) s += part[q * VP + tid];
      cur = xt + ((m + amax) + log(s));
      la[(size_t)t * V + tid] = cur;
    }
  }
  double m = block_max(cur);
  if (!(m > ninf())) m = 0.0;
  if (tid < VP) vec[tid] = tid < V ? exp(cur - m) : 0.0;
  __syncthreads();
  double zs = 0.0;
  for (int v = 0; v < V; v++) zs += vec[v];
  const double fcc = m + log(zs);
  if (tid == 0) p.fcc[b] = fcc;

  // ---- backward: thread (r0, ci) owns the pairs (r0 + PARTS * u, ci) ----
  const int ci = tid & (VP - 1), r0 = tid / VP;
  double acc[NPT];
#pragma unroll
  for (int u = 0; u < NPT; u++) acc[u] = 0.0;
  double lb = tid < V ? 0.0 : ninf();                  // log beta_t[tid]
  for (int t = n - 1; t >= 0; t--) {
    if (tid < V) grads[(size_t)t * V + tid] = (IO)(p.gscale * exp(la[(size_t)t * V + tid] + lb - fcc));
    if (t == 0) break;
    const double w = tid < V ? (double)x[(int64_t)t * p.sT + (int64_t)tid * p.sV] + lb : ninf();
    const double lap = ci < V ? la[(size_t)(t - 1) * V + ci] : ninf();
    double mb = block_max(w);
    if (!(mb > ninf())) mb = 0.0;
    if (tid < VP) vec[tid] = tid < V ? exp(w - mb) : 0.0;
    __syncthreads();
    const double f = ci < V ? exp(fmin(((lap + amax) + mb) - fcc, kAsgExpCap)) : 0.0;
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < NPT; u++) {
      const int j = r0 + PARTS * u;
      const double pr = eA[(size_t)j * PITCH + ci] * vec[j];
      s += pr;
      acc[u] += pr * f;
    }
    part[tid] = s;
    __syncthreads();
    if (tid < V) {
      s = 0.0;
#pragma unroll
      for (int q = 0; q < PARTS; q++) s += part[q * VP + tid];
      lb = (mb + amax) + log(s);
    }
  }
  double* gf = p.gf + (size_t)b * V * V;
#pragma unroll
  for (int u = 0; u < NPT; u++) {
    const int j = r0 + PARTS * u;
    if (j < V && ci < V) gf[(size_t)j * V + ci] = acc[u];
  }
}

template <typename IO>
__global__ __launch_bounds__(kLatticeThreads) void asg_fal_kernel(AsgParams p) {
  __shared__ double row[2][kAsgMaxS];                  // log alpha_t
  __shared__ double hrow[2][kAsgMaxS];                 // x_t[y_k] + log beta_t[k]
  __shared__ double post[2][kAsgMaxS];                 // the cells' posteriors of a frame
  __shared__ double ast[kAsgMaxS], aad[kAsgMaxS];      // A[y_k, y_k], A[y_k, y_{k-1}]
  __shared__ double stay[kAsgMaxS], adv[kAsgMaxS];     // the cells' arc posteriors summed over the frames
  __shared__ int y[kAsgMaxS], perm[kAsgMaxS];          // labels; cells in (label, k) order
  const int b = blockIdx.x, tid = threadIdx.x;
  const int V = p.V, Tmax = p.T, Sp = p.Sp;
  IO* grads = reinterpret_cast<IO*>(p.grads) + (size_t)b * Tmax * V;
  IO* tgr = reinterpret_cast<IO*>(p.tgrads) + (size_t)b * V * V;
  IO* loss = reinterpret_cast<IO*>(p.losses) + b;
  const int64_t Tq = p.x_len[b], Sq = p.t_len[b];
  const bool bad_len = Tq < 1 || Tq > Tmax || Sq < 1 || Sq > p.Smax;
  const int T = bad_len ? 0 : (int)Tq, S = bad_len ? 0 : (int)Sq;
  const int64_t* tg = p.targets + (int64_t)b * p.tgt_stride;
  int bad = bad_len;
  for (int i = tid; i < S; i += kLatticeThreads) bad |= tg[i] < 0 || tg[i] >= V;
  bad = __syncthreads_or(bad);
  if (bad || S > T) {                                  // bad: NaN everywhere; infeasible: +inf, NaN rows t < x_len, NaN slab
    const size_t rows = bad ? (size_t)Tmax : (size_t)T;
    for (size_t i = tid; i < rows * V; i += kLatticeThreads) grads[i] = (IO)NAN;
    for (int i = tid; i < V * V; i += kLatticeThreads) tgr[i] = (IO)NAN;
    if (tid == 0) *loss = bad ? (IO)NAN : (IO)INFINITY;
    return;
  }
  const IO* x = reinterpret_cast<const IO*>(p.x) + (int64_t)b * p.sB;
  const IO* At = reinterpret_cast<const IO*>(p.trans);
  double* fa = p.fa + (size_t)b * Tmax * Sp;
  const double fcc = p.fcc[b];

  for (int k = tid; k < S; k += kLatticeThreads) {
    const int u = (int)tg[k];
    y[k] = u;
    ast[k] = (double)At[u * V + u];
    aad[k] = k > 0 ? (double)At[u * V + (int)tg[k - 1]] : ninf();
  }
  __syncthreads();
  for (int k = tid; k < S; k += kLatticeThreads) {     // rank sort by (label, k)
    const int u = y[k];
    int r = 0;
    for (int i = 0; i < S; i++) { const int w = y[i]; r += (w < u) | ((w == u) & (i < k)); }
    perm[r] = k;
  }

  // ---- forward ----
#pragma unroll
  for (int c = 0; c < 2; c++) {
    const int k = tid + c * kLatticeThreads;
    if (k < S) {
      const double a = k == 0 ? (double)x[(int64_t)y[0] * p.sV] : ninf();
      row[0][k] = a; fa[k] = a;
    }
  }
  __syncthreads();
  for (int t = 1; t < T; t++) {
    const double* P = row[(t + 1) & 1];
    double* Q = row[t & 1];
#pragma unroll
    for (int c = 0; c < 2; c++) {
      const int k = tid + c * kLatticeThreads;
      if (k < S) {
        const double xt = (double)x[(int64_t)t * p.sT + (int64_t)y[k] * p.sV];
        const double a = lse2(P[k] + ast[k], k > 0 ? P[k - 1] + aad[k] : ninf()) + xt;
        Q[k] = a; fa[(size_t)t * Sp + k] = a;
      }
    }
    __syncthreads();
  }
  const double fal = row[(T - 1) & 1][S - 1];
  if (tid == 0) *loss = (IO)(fcc - fal);

  // ---- backward ----
  double sacc[2] = {0.0, 0.0}, aacc[2] = {0.0, 0.0};
  for (int t = T - 1; t >= 0; t--) {
    const double* H = hrow[(t + 1) & 1];
    double* Hn = hrow[t & 1];
    double* po = post[t & 1];
#pragma unroll
    for (int c = 0; c < 2; c++) {
      const int k = tid + c * kLatticeThreads;
      if (k < S) {
        const double xt = (double)x[(int64_t)t * p.sT + (int64_t)y[k] * p.sV];
        double bt;
        if (t == T - 1) bt = k == S - 1 ? 0.0 : ninf();
        else bt = lse2(ast[k] + H[k], k + 1 < S ? aad[k + 1] + H[k + 1] : ninf());
        const double h = xt + bt;
        Hn[k] = h;
        po[k] = exp((fa[(size_t)t * Sp + k] + bt) - fal);
        if (t > 0) {
          const double* ap = fa + (size_t)(t - 1) * Sp;
          sacc[c] += exp(((ap[k] + ast[k]) + h) - fal);
          if (k > 0) aacc[c] += exp(((ap[k - 1] + aad[k]) + h) - fal);
        }
      }
    }
    __syncthreads();
    for (int q = tid; q < S; q += kLatticeThreads) {   // grad[t, u] for the distinct labels u, their cells in cell order
      const int u = y[perm[q]];
      if (q > 0 && y[perm[q - 1]] == u) continue;
      double a = 0.0;
      for (int i = q; i < S && y[perm[i]] == u; i++) a += po[perm[i]];
      IO* g = grads + (size_t)t * V + u;
      *g = (IO)((double)*g - p.gscale * a);
    }
  }
#pragma unroll
  for (int c = 0; c < 2; c++) {
    const int k = tid + c * kLatticeThreads;
    if (k < S) { stay[k] = sacc[c]; adv[k] = aacc[c]; }
  }
  __syncthreads();
  const double* gf = p.gf + (size_t)b * V * V;
  for (int e = tid; e < V * V; e += kLatticeThreads) {  // one owner per entry, the cells in increasing k
    const int j = e / V, i = e - j * V;
    double s = 0.0;
    for (int k = 0; k < S; k++) {
      if (y[k] != j) continue;
      if (i == j) s += stay[k];
      if (k > 0 && y[k - 1] == i) s += adv[k];
    }
    tgr[e] = (IO)(p.gscale * (gf[e] - s));
  }
}

constexpr size_t asg_vit_lds(int VP) {
  return sizeof(double) * ((size_t)VP * (VP + 1) + 2 * VP + kLatticeThreads) + sizeof(int) * kLatticeThreads + 64;
}

template <typename IO, int VP>
__global__ __launch_bounds__(kLatticeThreads) void asg_viterbi_kernel(AsgVitParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int NPT = VP * VP / kLatticeThreads;
  constexpr int PARTS = kLatticeThreads / VP;
  constexpr int PITCH = VP + 1;
  double* A = reinterpret_cast<double*>(smem);         // [VP][PITCH], -inf outside V x V
  double* d = A + (size_t)VP * PITCH;                  // [2][VP]
  double* pv = d + 2 * VP;                             // [256] the parts' maxima
  int* pi = reinterpret_cast<int*>(pv + kLatticeThreads);   // [256] and where they were met
  __shared__ int s_len;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int V = p.V, Tmax = p.T;
  int64_t* path = p.path + (size_t)b * Tmax;
  int64_t* coll = p.collapsed + (size_t)b * Tmax;
  const int64_t Tq = p.x_len[b];
  if (Tq < 1 || Tq > Tmax) {
    for (int t = tid; t < Tmax; t += kLatticeThreads) { path[t] = p.pad; coll[t] = 0; }
    if (tid == 0) { p.scores[b] = NAN; p.lengths[b] = 0; }
    return;
  }
  const int n = (int)Tq;
  const IO* x = reinterpret_cast<const IO*>(p.x) + (int64_t)b * p.sB;
  const IO* At = reinterpret_cast<const IO*>(p.trans);
  unsigned char* bp = p.bp + (size_t)b * Tmax * V;
  for (int e = tid; e < VP * VP; e += kLatticeThreads) {
    const int j = e / VP, i = e % VP;
    A[(size_t)j * PITCH + i] = (j < V && i < V) ? (double)At[j * V + i] : ninf();
  }
  if (tid < VP) d[tid] = tid < V ? (double)x[(int64_t)tid * p.sV] : ninf();
  for (int t = n + tid; t < Tmax; t += kLatticeThreads) path[t] = p.pad;
  __syncthreads();
  const int rj = tid & (VP - 1), rp = tid / VP;
  for (int t = 1; t < n; t++) {
    const double* D = d + ((t + 1) & 1) * VP;
    double* Dn = d + (t & 1) * VP;
    const double xt = tid < V ? (double)x[(int64_t)t * p.sT + (int64_t)tid * p.sV] : 0.0;
    double best = ninf();
    int bi = rp * NPT;
#pragma unroll
    for (int u = 0; u < NPT; u++) {                    // ties: the lowest i
      const int i = rp * NPT + u;
      const double v = D[i] + A[(size_t)rj * PITCH + i];
      if (v > best) { best = v; bi = i; }
    }
    pv[tid] = best; pi[tid] = bi;
    __syncthreads();
    if (tid < V) {
      best = pv[tid]; bi = pi[tid];
#pragma unroll
      for (int q = 1; q < PARTS; q++) {
        const double v = pv[q * VP + tid];
        if (v > best) { best = v; bi = pi[q * VP + tid]; }
      }
      Dn[tid] = best + xt;
      bp[(size_t)t * V + tid] = (unsigned char)bi;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double* D = d + ((n - 1) & 1) * VP;
    double best = D[0];
    int j = 0;
    for (int v = 1; v < V; v++) if (D[v] > best) { best = D[v]; j = v; }
    p.scores[b] = best;
    path[n - 1] = j;
    for (int t = n - 1; t >= 1; t--) { j = bp[(size_t)t * V + j]; path[t - 1] = j; }
    int len = 0;
    int64_t prev = -1;
    for (int t = 0; t < n; t++) {
      const int64_t c = path[t];
      if (c != prev) coll[len++] = c;
      prev = c;
    }
    p.lengths[b] = len;
    s_len = len;
  }
  __syncthreads();
  for (int t = s_len + tid; t < Tmax; t += kLatticeThreads) coll[t] = 0;
}

int asg_vp(int V) { return V <= 32 ? 32 : V <= 64 ? 64 : 128; }

// Workspace of the loss (offsets from its 256-byte aligned start)
struct AsgLayout { size_t la, gf, fcc, fa, total; int Sp; };
AsgLayout asg_layout(int B, int T, int V, int Smax) {
  AsgLayout l{};
  l.Sp = Smax > 1 ? Smax : 1;
  l.la = 0;
  l.gf = align_up((size_t)B * T * V * sizeof(double), 256);
  l.fcc = l.gf + align_up((size_t)B * V * V * sizeof(double), 256);
  l.fa = l.fcc + align_up((size_t)B * sizeof(double), 256);
  l.total = l.fa + align_up((size_t)B * T * l.Sp * sizeof(double), 256);
  return l;
}
bool asg_served(int V, int Smax) { return V >= 1 && V <= kAsgMaxV && Smax >= 0 && Smax <= kAsgMaxS; }

template <typename IO>
int asg_launch(const LossArgs& a, const AsgParams& p) {
  void (*fcc)(AsgParams) = nullptr;
  const int VP = asg_vp(a.V);
  if (VP == 32) fcc = asg_fcc_kernel<IO, 32>;
  else if (VP == 64) fcc = asg_fcc_kernel<IO, 64>;
  else fcc = asg_fcc_kernel<IO, 128>;
  const size_t lds = asg_dense_lds(VP);
  E2E_HIP_CHECK(allow_dynamic_lds(reinterpret_cast<const void*>(fcc), (int)lds), "hipFuncSetAttribute");
  hipLaunchKernelGGL(fcc, dim3(a.B), dim3(kLatticeThreads), lds, a.stream, p);
  E2E_HIP_CHECK(hipGetLastError(), "asg_fcc_kernel launch");
  hipLaunchKernelGGL(asg_fal_kernel<IO>, dim3(a.B), dim3(kLatticeThreads), 0, a.stream, p);
  E2E_HIP_CHECK(hipGetLastError(), "asg_fal_kernel launch");
  return E2E_OK;
}

template <typename IO>
int asg_viterbi_launch(const AsgVitParams& p, hipStream_t stream) {
  void (*k)(AsgVitParams) = nullptr;
  const int VP = asg_vp(p.V);
  if (VP == 32) k = asg_viterbi_kernel<IO, 32>;
  else if (VP == 64) k = asg_viterbi_kernel<IO, 64>;
  else k = asg_viterbi_kernel<IO, 128>;
  const size_t lds = asg_vit_lds(VP);
  E2E_HIP_CHECK(allow_dynamic_lds(reinterpret_cast<const void*>(k), (int)lds), "hipFuncSetAttribute");
  hipLaunchKernelGGL(k, dim3(p.B), dim3(kLatticeThreads), lds, stream, p);
  E2E_HIP_CHECK(hipGetLastError(), "asg_viterbi_kernel launch");
  return E2E_OK;
}

}  // namespace
}  // namespace e2e

using namespace e2e;

extern "C" int e2e_asg_max_labels(void) { return kAsgMaxV; }
extern "C" int e2e_asg_max_target_length(void) { return kAsgMaxS; }

extern "C" size_t e2e_asg_workspace_bytes(int B, int T, int V, int Smax, int dtype) {
  (void)dtype;
  if (B < 0 || T < 1 || !asg_served(V, Smax)) return 0;
  return asg_layout(B, T, V, Smax).total + 256;
}

extern "C" int e2e_asg_fwd_bwd(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV, const void* transitions,
                               const int64_t* targets, int64_t tgt_stride, const int64_t* x_len, const int64_t* t_len,
                               int B, int T, int V, int Smax, void* losses, void* grads, void* tgrads, void* workspace,
                               size_t workspace_bytes, void* stream, const e2e_ctc_loss_opts* opts) {
  LossArgs a{x, dtype, 1, sB, sT, sV, targets, tgt_stride, x_len, t_len,
             B, T, V, Smax, 0, losses, grads, workspace, workspace_bytes, (hipStream_t)stream};
  int rc = lattice_check_args(a, opts);
  if (rc != E2E_OK) return rc;
  if (B > 0 && (!transitions || !tgrads)) { set_error("null pointer argument"); return E2E_ERR_ARG; }
  if (!asg_served(V, Smax)) {
    set_error("ASG: V=%d, Smax=%d; the kernels serve alphabets of up to %d columns and targets of up to %d labels", V, Smax, kAsgMaxV, kAsgMaxS);
    return E2E_ERR_UNSUPPORTED;
  }
  if (a.reduction != E2E_REDUCE_NONE) { set_error("ASG: no fused reduction; sum the losses"); return E2E_ERR_UNSUPPORTED; }
  const AsgLayout l = asg_layout(B, T, V, Smax);
  LatticeLayout need{};
  need.total = l.total;
  rc = lattice_workspace(a, need);
  if (rc != E2E_OK || B == 0) return rc;
  unsigned char* ws = reinterpret_cast<unsigned char*>(a.ws);
  AsgParams p;
  p.x = x; p.sB = sB; p.sT = sT; p.sV = sV; p.trans = transitions;
  p.targets = targets; p.tgt_stride = tgt_stride; p.x_len = x_len; p.t_len = t_len;
  p.B = B; p.T = T; p.V = V; p.Smax = Smax; p.Sp = l.Sp;
  p.gscale = a.grad_scale; p.losses = losses; p.grads = grads; p.tgrads = tgrads;
  p.la = reinterpret_cast<double*>(ws + l.la); p.gf = reinterpret_cast<double*>(ws + l.gf);
  p.fcc = reinterpret_cast<double*>(ws + l.fcc); p.fa = reinterpret_cast<double*>(ws + l.fa);
  return dtype == E2E_F32 ? asg_launch<float>(a, p) : asg_launch<double>(a, p);
}

extern "C" size_t e2e_asg_viterbi_workspace_bytes(int B, int T, int V) {
  if (B < 0 || T < 1 || V < 1 || V > kAsgMaxV) return 0;
  return align_up((size_t)B * T * V, 256) + 256;
}

extern "C" int e2e_asg_viterbi(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV, const void* transitions,
                               const int64_t* x_len, int B, int T, int V, int64_t* path, int64_t pad_value, double* scores,
                               int64_t* collapsed, int64_t* lengths, void* workspace, size_t workspace_bytes, void* stream) {
  if (dtype != E2E_F32 && dtype != E2E_F64) { set_error("dtype must be E2E_F32 or E2E_F64 (up-cast 16-bit inputs)"); return E2E_ERR_ARG; }
  if (B < 0 || T < 1 || V < 1) { set_error("bad sizes B=%d T=%d V=%d", B, T, V); return E2E_ERR_ARG; }
  if (B > 0 && (!x || !transitions || !x_len || !path || !scores || !collapsed || !lengths)) { set_error("null pointer argument"); return E2E_ERR_ARG; }
  if (V > kAsgMaxV) { set_error("ASG best path: V=%d; the kernel serves alphabets of up to %d columns", V, kAsgMaxV); return E2E_ERR_UNSUPPORTED; }
  const size_t need = align_up((size_t)B * T * V, 256);
  void* ws = workspace;
  size_t left = workspace_bytes;
  if (!align_workspace(ws, left) || left < need) { set_error("workspace too small: need %zu", need + 256); return E2E_ERR_WORKSPACE; }
  if (B == 0) return E2E_OK;
  AsgVitParams p{x, sB, sT, sV, transitions, x_len, B, T, V, path, pad_value, scores, collapsed, lengths,
                 reinterpret_cast<unsigned char*>(ws)};
  return dtype == E2E_F32 ? asg_viterbi_launch<float>(p, (hipStream_t)stream) : asg_viterbi_launch<double>(p, (hipStream_t)stream);
}
