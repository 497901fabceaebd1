// Gram-CTC decoding (the definition: include/e2e_ctc.h, beside the Gram-CTC loss).
//
// Greedy: the arg-max / collapse kernel of ctc_greedy.hip with blank 0 gives the collapsed columns; gram_expand_kernel
// turns them into base ids (a prefix sum of the grams' lengths over the columns, then a scatter).
//
// Beam search: one workgroup per utterance.  The beam's members (up to 128 prefixes, each with its max_order + 1 slots)
// live in LDS, double buffered.  A frame's candidates meet in an open-addressing table of 64-bit prefix keys in the
// workspace: every member and every (member, column) pair with a non-zero share claims or finds its key with a 64-bit
// compare-and-swap and pushes its own id on the entry's list with an exchange.  Nothing is added there: a share is a
// function of the pair (src * y[c]) and is recomputed by whoever walks the list.  A (prefix, slot) receives at most its
// stay share and one extension share, so a slot is the sum of two numbers and a total the sum of the slots in the order
// 0 .. max_order -- the same bits whatever order the pairs arrived in.  The per-frame cut first drops what cannot matter
// (a full beam's members are W candidates themselves: nothing below the least of their new totals survives); the select
// and the ranking are beam_cut.h's, the select on the bits of the totals (positive doubles order as integers), and the
// survivors become the next members in the order of their ranks.  The table is cleared entry by entry from the frame's
// candidate list.  The read-out walks the (parent node, column) pool backwards and expands the grams.
#include "beam_cut.h"

namespace e2e {

int launch_greedy(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len,
                  int B, int T, int V, int blank, int64_t* out, int64_t* out_len, hipStream_t stream);

namespace {

constexpr int kExpandThreads = 256;
constexpr int kBeamThreads = 1024;
constexpr int kMaxK = 8;                   // longest gram
constexpr int kMaxPairs = 131072;          // beam_width * V

__device__ __forceinline__ int order_of(const int32_t* gram_len, int c, int K) {
  const int k = gram_len[c];
  return k < 1 ? 1 : (k > K ? K : k);
}

// ---- greedy: columns -> base ids ----------------------------------------------------------------------------------
struct GramExpandParams {
  const int64_t* cols; const int64_t* cols_len; const int32_t* gram_ids; const int32_t* gram_len;
  int T, V, K; int64_t* out; int64_t* out_len;
};

__global__ __launch_bounds__(kExpandThreads) void gram_expand_kernel(GramExpandParams p) {
  __shared__ int wave_tot[kExpandThreads / 64];
  __shared__ int carry;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t* cols = p.cols + (int64_t)b * p.T;
  const int64_t width = (int64_t)p.T * p.K;
  int64_t* out = p.out + (int64_t)b * width;
  const int64_t nq = p.cols_len[b];
  const int n = nq < 0 ? 0 : (nq > p.T ? p.T : (int)nq);
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += kExpandThreads) {
    const int i = i0 + tid;
    int c = 0, len = 0;
    if (i < n) {
      const int64_t cq = cols[i];
      c = (cq >= 1 && cq < p.V) ? (int)cq : 0;
      len = c ? order_of(p.gram_len, c, p.K) : 0;
    }
    int incl = len;
    for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o, 64); if (lane >= o) incl += v; }
    if (lane == 63) wave_tot[wid] = incl;
    __syncthreads();
    int base = carry + incl - len, total = 0;
    for (int w = 0; w < kExpandThreads / 64; w++) { if (w < wid) base += wave_tot[w]; total += wave_tot[w]; }
    for (int j = 0; j < len; j++) out[base + j] = (int64_t)p.gram_ids[c * kMaxK + j];
    __syncthreads();
    if (tid == 0) carry += total;
    __syncthreads();
  }
  const int total = carry;
  for (int64_t i = total + tid; i < width; i += kExpandThreads) out[i] = 0;
  if (tid == 0) p.out_len[b] = total;
}

// ---- beam search --------------------------------------------------------------------------------------------------
struct Entry { unsigned long long key; int head; int pad; };      // key 0: free

struct Members {
  double p[kMaxK + 1][kMaxW];        // slot masses; slot 0 the blank's
  int col[kMaxK + 1][kMaxW];         // column of slot k >= 1 (0 while the slot is empty)
  unsigned long long key[kMaxW];
  double tot[kMaxW];                 // p[0] + p[1] + ... + p[K], in that order
  int node[kMaxW], len[kMaxW];
};

struct GramBeamParams {
  const void* lp; int dtype; int64_t sB, sT, sV; const int64_t* x_len;
  int B, T, V; const int32_t* gram_ids; const int32_t* gram_len; int K, W, nbest;
  int64_t* out; int64_t max_out; int64_t* out_len; int64_t* n_hyp; double* scores;
  unsigned char* ws; size_t per_utt, off_table, off_next, off_list, off_tot, off_sval, off_spos, off_nodes; int logH;
};

// the mass an extension of member m by column c (order k) starts from: every slot but a slot k that holds c itself
__device__ __forceinline__ double ext_source(const Members& M, int m, int k, int c, int K) {
  if (M.col[k][m] != c || !(M.p[k][m] > 0.0)) return M.tot[m];
  double s = 0.0;
  for (int kk = 0; kk <= K; kk++) if (kk != k) s += M.p[kk][m];
  return s;
}

struct Eval {
  double s[kMaxK + 1];               // the candidate's slots
  int c[kMaxK + 1];                  // their columns
  int stay;                          // the member that is this prefix already, or -1
  int pair;                          // the smallest (member, column) id that extends to it
};

// walks a candidate's list of ids (m * V + c; c == 0: member m itself) and recomputes its slots
__device__ __forceinline__ void eval_list(Eval& E, const Members& M, int head, const int* next, const double* y,
                                          const int32_t* gram_len, unsigned V, int K, unsigned n_ids) {
#pragma unroll
  for (int k = 0; k <= kMaxK; k++) { E.s[k] = 0.0; E.c[k] = 0; }
  E.stay = -1; E.pair = 0x7fffffff;
  int id = head;
  for (int steps = 0; steps < 2 * (kMaxK + 1) && (unsigned)id < n_ids; steps++) {
    const unsigned m = (unsigned)id / V, c = (unsigned)id - m * V;
    if (c == 0) {
      E.stay = (int)m;
      E.s[0] += M.tot[m] * y[0];
#pragma unroll
      for (int k = 1; k <= kMaxK; k++)
        if (k <= K) {
          const double pk = M.p[k][m];
          if (pk > 0.0) { const int ck = M.col[k][m]; E.s[k] += pk * y[ck]; if (!E.c[k]) E.c[k] = ck; }
        }
    } else {
      const int k = order_of(gram_len, (int)c, K);
      const double v = ext_source(M, (int)m, k, (int)c, K) * y[c];
#pragma unroll
      for (int kk = 1; kk <= kMaxK; kk++) if (kk == k) { E.s[kk] += v; E.c[kk] = (int)c; }
      if (id < E.pair) E.pair = id;
    }
    id = next[id];
  }
}

__device__ __forceinline__ double eval_total(const Eval& E, int K) {
  double t = 0.0;
#pragma unroll
  for (int k = 0; k <= kMaxK; k++) if (k <= K) t += E.s[k];
  return t;
}

__global__ __launch_bounds__(kBeamThreads) void gram_beam_kernel(GramBeamParams p) {
  __shared__ Members mem[2];
  __shared__ BeamCut cut;
  __shared__ int n_cand, n_surv, overflow;
  __shared__ unsigned long long sh_floor;
  __shared__ double sh_best;

  const int b = blockIdx.x, tid = threadIdx.x;
  const int V = p.V, K = p.K, W = p.W;
  const unsigned n_ids = (unsigned)W * (unsigned)V;
  unsigned char* ws = p.ws + (size_t)b * p.per_utt;
  double* y = reinterpret_cast<double*>(ws);
  Entry* table = reinterpret_cast<Entry*>(ws + p.off_table);
  int* next = reinterpret_cast<int*>(ws + p.off_next);
  int* list = reinterpret_cast<int*>(ws + p.off_list);
  double* ctot = reinterpret_cast<double*>(ws + p.off_tot);
  unsigned long long* sval = reinterpret_cast<unsigned long long*>(ws + p.off_sval);
  int* spos = reinterpret_cast<int*>(ws + p.off_spos);
  int2* nodes = reinterpret_cast<int2*>(ws + p.off_nodes);
  const unsigned H = 1u << p.logH, hmask = H - 1u;
  const int64_t Tq = p.x_len[b];
  const int Tb = Tq < 0 ? 0 : (Tq > p.T ? p.T : (int)Tq);

  for (unsigned i = tid; i < H; i += kBeamThreads) { table[i].key = 0ull; table[i].head = -1; }
  if (tid == 0) {
    for (int k = 0; k <= kMaxK; k++) { mem[0].p[k][0] = k == 0 ? 1.0 : 0.0; mem[0].col[k][0] = 0; }
    mem[0].key[0] = kKeyBasis; mem[0].tot[0] = 1.0; mem[0].node[0] = 0; mem[0].len[0] = 0;
    nodes[0] = make_int2(-1, 0);
    overflow = 0;
  }
  __syncthreads();

  int cur = 0, n_mem = 1;
  long long esum = 0;                                           // exponents taken out of the frames so far
  for (int t = 0; t < Tb && n_mem > 0; t++) {
    const Members& M = mem[cur];
    Members& N = mem[cur ^ 1];
    // ---- the frame's probabilities ----
    {
      const int64_t row = (int64_t)b * p.sB + (int64_t)t * p.sT;
      for (int c = tid; c < V; c += kBeamThreads) {
        const int64_t at = row + (int64_t)c * p.sV;
        const double v = p.dtype == E2E_F32 ? (double)reinterpret_cast<const float*>(p.lp)[at]
                                            : reinterpret_cast<const double*>(p.lp)[at];
        y[c] = exp(v);
      }
    }
    if (tid == 0) { n_cand = 0; n_surv = 0; cut.n_sel = 0; sh_floor = ~0ull; }
    __syncthreads();
    // ---- members and (member, column) pairs meet at their prefix's key ----
    const unsigned n_now = (unsigned)n_mem * (unsigned)V;
    for (unsigned id = tid; id < n_now; id += kBeamThreads) {
      const unsigned m = id / (unsigned)V, c = id - m * (unsigned)V;
      unsigned long long key = M.key[m];
      bool go = true;
      if (c != 0) {
        const int k = order_of(p.gram_len, (int)c, K);
        go = ext_source(M, (int)m, k, (int)c, K) * y[c] > 0.0;
        if (go) for (int j = 0; j < k; j++) key = (key ^ (unsigned long long)(unsigned)p.gram_ids[c * kMaxK + j]) * kKeyPrime;
      }
      if (!go) continue;
      if (key == 0ull) key = 1ull;                               // (0 marks a free entry)
      unsigned h = (unsigned)((key * kHashMul) >> (64 - p.logH));
      bool found = false;
      for (unsigned probe = 0; probe < H; probe++) {
        const unsigned long long old = atomicCAS(&table[h].key, 0ull, key);
        if (old == 0ull) { const int pos = atomicAdd(&n_cand, 1); if ((unsigned)pos < n_ids) list[pos] = (int)h; found = true; break; }
        if (old == key) { found = true; break; }
        h = (h + 1u) & hmask;
      }
      if (found) next[id] = atomicExch(&table[h].head, (int)id);
      else overflow = 1;
    }
    __syncthreads();
    // ---- every candidate's total ----
    const int nc = min(n_cand, (int)n_ids);
    for (int pos = tid; pos < nc; pos += kBeamThreads) {
      const int e = list[pos];
      const int head = __hip_atomic_load(&table[e].head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      Eval E;
      eval_list(E, M, head, next, y, p.gram_len, (unsigned)V, K, n_ids);
      const double tot = eval_total(E, K);
      ctot[pos] = tot;
      if (E.stay >= 0) atomicMin(&sh_floor, tot > 0.0 ? (unsigned long long)__double_as_longlong(tot) : 0ull);
    }
    __syncthreads();
    // ---- an exact filter: a full beam's members are W candidates themselves, so nothing below the least of them can
    //      make the cut; what is left (usually a few times W) is what the selection reads ----
    const unsigned long long floor_bits = n_mem == W ? sh_floor : 0ull;
    for (int pos = tid; pos < nc; pos += kBeamThreads) {
      const double tot = ctot[pos];
      const unsigned long long v = (unsigned long long)__double_as_longlong(tot);
      if (!(tot > 0.0) || v < floor_bits) continue;              // (NaN totals, from NaN inputs, are no members either)
      const int j = atomicAdd(&n_surv, 1);
      sval[j] = v; spos[j] = pos;
    }
    __syncthreads();
    // ---- the cut: the W largest totals, exactly equal ones by ascending key ----
    beam_cut<kBeamThreads>(cut, sval, spos, n_surv, W,
        [&](int pos) { return __hip_atomic_load(&table[list[pos]].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
        [](unsigned long long v) { return __longlong_as_double((long long)v); });
    __syncthreads();
    const int ns = beam_cut_count(cut, W);
    if (ns == 0) {                                               // every path has probability 0: no hypothesis is left
      for (int pos = tid; pos < nc; pos += kBeamThreads) { Entry& en = table[list[pos]]; en.key = 0ull; en.head = -1; }
      n_mem = 0;
      __syncthreads();
      break;
    }
    // ---- rank the survivors: they become the members in that order ----
    beam_cut_rank(cut, ns);
    if (tid < ns && cut.sel_rank[tid] == 0) sh_best = cut.sel_tot[tid];
    __syncthreads();
    int ex = 0;
    (void)frexp(sh_best, &ex);                                   // best = f * 2^ex, f in [0.5, 1)
    if (tid < ns) {
      const int pos = cut.sel_pos[tid], r = cut.sel_rank[tid];
      const int head = __hip_atomic_load(&table[list[pos]].head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      Eval E;
      eval_list(E, M, head, next, y, p.gram_len, (unsigned)V, K, n_ids);
      double tot = 0.0;
#pragma unroll
      for (int k = 0; k <= kMaxK; k++) {
        const double pk = k <= K ? ldexp(E.s[k], -ex) : 0.0;
        N.p[k][r] = pk; N.col[k][r] = (k >= 1 && pk > 0.0) ? E.c[k] : 0;
        if (k <= K) tot += pk;
      }
      N.tot[r] = tot; N.key[r] = cut.sel_key[tid];
      if (E.stay >= 0) { N.node[r] = M.node[E.stay]; N.len[r] = M.len[E.stay]; }
      else {
        const unsigned pid = (unsigned)E.pair < n_ids ? (unsigned)E.pair : 0u;
        const unsigned pm = pid / (unsigned)V, pc = pid - pm * (unsigned)V;
        const int node = 1 + t * W + r;
        nodes[node] = make_int2(M.node[pm], (int)pc);
        N.node[r] = node; N.len[r] = M.len[pm] + order_of(p.gram_len, (int)pc, K);
      }
    }
    __syncthreads();                                             // (the lists above are read to the end before they go)
    // ---- free the frame's entries ----
    for (int pos = tid; pos < nc; pos += kBeamThreads) { Entry& en = table[list[pos]]; en.key = 0ull; en.head = -1; }
    esum += ex; n_mem = ns; cur ^= 1;
    __syncthreads();
  }

  // ---- read-out: the first nbest members, ranked already ----
  const Members& F = mem[cur];
  const int nbest = p.nbest;
  const int64_t max_out = p.max_out;
  int64_t* out = p.out + (int64_t)b * nbest * max_out;
  if (tid < nbest) {
    int64_t* row = out + (int64_t)tid * max_out;
    int len = 0; double score = -__builtin_huge_val();
    if (tid < n_mem) {
      len = F.len[tid];
      score = log(F.tot[tid]) + (double)esum * 0.6931471805599453094;
      int at = len, node = F.node[tid];
      for (int hops = 0; node > 0 && hops <= p.T; hops++) {
        const int2 nd = nodes[node];
        const int k = order_of(p.gram_len, nd.y, K);
        for (int j = k - 1; j >= 0; j--) { --at; if (at >= 0 && at < max_out) row[at] = (int64_t)p.gram_ids[nd.y * kMaxK + j]; }
        node = nd.x;
      }
    }
    cut.sel_pos[tid] = len;
    p.out_len[(int64_t)b * nbest + tid] = len;
    p.scores[(int64_t)b * nbest + tid] = score;
  }
  __syncthreads();
  for (int j = 0; j < nbest; j++) {
    int64_t* row = out + (int64_t)j * max_out;
    for (int64_t i = cut.sel_pos[j] + tid; i < max_out; i += kBeamThreads) row[i] = 0;
  }
  if (tid == 0) p.n_hyp[b] = overflow ? -1 : (n_mem < nbest ? n_mem : nbest);
}

struct BeamLayout { size_t per_utt, off_table, off_next, off_list, off_tot, off_sval, off_spos, off_nodes; int logH; };

bool beam_layout(int T, int V, int K, int W, BeamLayout& L) {
  if (T < 1 || V < 1 || K < 1 || K > kMaxK || W < 1 || W > kMaxW || (int64_t)W * V > kMaxPairs || T > (1 << 22)) return false;
  const size_t ids = (size_t)W * V;
  int logH = 6;
  while (((size_t)1 << logH) < 2 * ids) logH++;
  size_t at = align_up((size_t)V * 8, 256);
  L.off_table = at; at += align_up(((size_t)1 << logH) * sizeof(Entry), 256);
  L.off_next = at; at += align_up(ids * 4, 256);
  L.off_list = at; at += align_up(ids * 4, 256);
  L.off_tot = at; at += align_up(ids * 8, 256);
  L.off_sval = at; at += align_up(ids * 8, 256);
  L.off_spos = at; at += align_up(ids * 4, 256);
  L.off_nodes = at; at += align_up(((size_t)W * ((size_t)T + 1) + 1) * 8, 256);
  L.per_utt = at; L.logH = logH;
  return true;
}

}  // namespace
}  // namespace e2e

using namespace e2e;

extern "C" {

int e2e_gram_ctc_greedy(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len,
                        int B, int T, int V, const int32_t* gram_ids, const int32_t* gram_len, int max_order,
                        int64_t* out, int64_t* out_len, int64_t* cols, int64_t* cols_len, void* stream) {
  if (dtype != E2E_F32 && dtype != E2E_F64 && !dtype_is_16bit(dtype)) { set_error("dtype must be E2E_F32, E2E_F64, E2E_F16 or E2E_BF16"); return E2E_ERR_ARG; }
  if (B < 0 || T < 1 || V < 1) { set_error("bad sizes B=%d T=%d V=%d", B, T, V); return E2E_ERR_ARG; }
  if (max_order < 1 || max_order > kMaxK) { set_error("max_order %d is not in [1, %d]", max_order, kMaxK); return E2E_ERR_ARG; }
  if ((int64_t)T * max_order > 0x7fffffffLL) { set_error("T * max_order = %lld does not fit", (long long)T * max_order); return E2E_ERR_UNSUPPORTED; }
  if (B > 0 && (!x || !x_len || !gram_ids || !gram_len || !out || !out_len || !cols || !cols_len)) { set_error("null pointer argument"); return E2E_ERR_ARG; }
  if (B == 0) return E2E_OK;
  const int rc = launch_greedy(x, dtype, sB, sT, sV, x_len, B, T, V, 0, cols, cols_len, (hipStream_t)stream);
  if (rc != E2E_OK) return rc;
  GramExpandParams p{cols, cols_len, gram_ids, gram_len, T, V, max_order, out, out_len};
  hipLaunchKernelGGL(gram_expand_kernel, dim3(B), dim3(kExpandThreads), 0, (hipStream_t)stream, p);
  E2E_HIP_CHECK(hipGetLastError(), "gram_expand_kernel launch");
  return E2E_OK;
}

int e2e_gram_beam_max_width(int V, int max_order) {
  if (V < 1 || max_order < 1 || max_order > kMaxK) return 0;
  const int w = kMaxPairs / V;
  return w < kMaxW ? w : kMaxW;
}

size_t e2e_gram_beam_workspace_bytes(int B, int T, int V, int max_order, int beam_width) {
  BeamLayout L;
  if (B < 0 || !beam_layout(T, V, max_order, beam_width, L)) return 0;
  return (size_t)B * L.per_utt + 256;
}

int e2e_gram_ctc_beam_nbest(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len,
                            int B, int T, int V, const int32_t* gram_ids, const int32_t* gram_len, int max_order,
                            int beam_width, int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp,
                            double* scores, void* workspace, size_t workspace_bytes, void* stream) {
  if (dtype != E2E_F32 && dtype != E2E_F64) { set_error("dtype must be E2E_F32 or E2E_F64"); return E2E_ERR_ARG; }
  if (B < 0 || T < 1 || V < 1 || max_out < 0) { set_error("bad sizes B=%d T=%d V=%d max_out=%lld", B, T, V, (long long)max_out); return E2E_ERR_ARG; }
  if (max_order < 1 || max_order > kMaxK) { set_error("max_order %d is not in [1, %d]", max_order, kMaxK); return E2E_ERR_ARG; }
  if (beam_width < 1) { set_error("beam_width %d must be at least 1", beam_width); return E2E_ERR_ARG; }
  if (beam_width > e2e_gram_beam_max_width(V, max_order)) {
    set_error("beam_width %d exceeds e2e_gram_beam_max_width(V=%d, max_order=%d) = %d", beam_width, V, max_order,
              e2e_gram_beam_max_width(V, max_order));
    return E2E_ERR_UNSUPPORTED;
  }
  if (nbest < 1 || nbest > beam_width) { set_error("nbest=%d outside [1, beam_width=%d]", nbest, beam_width); return E2E_ERR_ARG; }
  BeamLayout L;
  if (!beam_layout(T, V, max_order, beam_width, L)) { set_error("T=%d frames are more than the search takes", T); return E2E_ERR_UNSUPPORTED; }
  if (B > 0 && (!lp || !x_len || !gram_ids || !gram_len || !out_len || !n_hyp || !scores || (max_out > 0 && !out))) {
    set_error("null pointer argument"); return E2E_ERR_ARG;
  }
  if (B == 0) return E2E_OK;
  if (!align_workspace(workspace, workspace_bytes) || workspace_bytes < (size_t)B * L.per_utt) {
    set_error("workspace too small: %zu bytes, e2e_gram_beam_workspace_bytes() = %zu", workspace_bytes, (size_t)B * L.per_utt + 256);
    return E2E_ERR_WORKSPACE;
  }
  GramBeamParams p{lp, dtype, sB, sT, sV, x_len, B, T, V, gram_ids, gram_len, max_order, beam_width, nbest,
                   out, max_out, out_len, n_hyp, scores, reinterpret_cast<unsigned char*>(workspace),
                   L.per_utt, L.off_table, L.off_next, L.off_list, L.off_tot, L.off_sval, L.off_spos, L.off_nodes, L.logH};
  hipLaunchKernelGGL(gram_beam_kernel, dim3(B), dim3(kBeamThreads), 0, (hipStream_t)stream, p);
  E2E_HIP_CHECK(hipGetLastError(), "gram_beam_kernel launch");
  return E2E_OK;
}

}  // extern "C"
