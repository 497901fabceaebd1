// Word-segmented CTC (CTCLossSegmented): the plan, the regrouping of frames into a batch of segments, and the way back.
//
// Replaces the Python loops of pytorch_end2end/modules/ctc_loss_segmented.py:43-146 upstream, which walk `.data[i]` of host
// copies frame by frame.  The alignment (e2e_ctc_align) and the segments' losses (e2e_ctc_loss_fwd_bwd) are the existing
// kernels; what is here is what lies between them (the definition: include/e2e_ctc.h):
//
//   plan     match     one sub-wave group of lanes per frame: arg-max of the logits row (ties as e2e_ctc_greedy), compared
//                      with the alignment; one byte of flags per frame.
//            bounds    one workgroup per utterance.  The automaton of upstream's loop resets at every well-recognised space,
//                      so between two of them it is a pair of counts: a space qualifies iff no frame since the previous
//                      recognised space mismatches and at least min_word_length label runs start there.  That is a
//                      segmented scan (each thread folds a contiguous stretch of frames, the workgroup scans the 256
//                      folds); the boundaries are a SET of frames (frame 0, the qualifying spaces, the recognised space
//                      before each, the last frame), so they are marked, counted and ranked, never appended.  The segments
//                      of an utterance are staged at its own frames' slots.
//            scan      per-utterance counts -> first-segment offsets (one workgroup; no atomics decide an order).
//            table     one wave per segment: the record moves to its place in the table; a chunk's target -- runs of the
//                      alignment collapsed, blanks dropped -- is compacted by ballot into the pool at the chunk's own start.
//            summary   counts per kind and the sizes the host needs, in the table's first words.
//   gather   one workgroup row per listed segment: its frames copied into a dense zero-padded batch (flat, coalesced when the
//            logits rows are contiguous), its target and lengths beside them.
//   finish   a gathered batch's gradient copied back to the segment's frames (contiguous in (B,T,V): a flat copy); then, once,
//            the frames no gathered segment owns -- single-frame segments in closed form in f64, padded frames 0 -- and the
//            sum of every utterance's segment losses in table order.
#include "common.h"

namespace e2e {
namespace {

constexpr int kThreads = 256;
constexpr int kHdr = E2E_WORDSEG_HEADER;

// torch CPU argmax semantics: first maximum wins, NaN counts as the maximum (as ctc_greedy.hip)
template <typename F>
__device__ __forceinline__ bool better(F cand, int cand_i, F best, int best_i) {
  const bool cn = cand != cand, bn = best != best;
  if (bn) return cn && cand_i < best_i;
  if (cn) return true;
  return cand > best || (cand == best && cand_i < best_i);
}

// the workspace: per-frame state that lives from the plan to the finish
struct Work {
  unsigned char* flags;   // [B*T] bit 0 mismatch, bit 1 recognised space, bit 2 a label run starts here (recognised)
  unsigned char* bnd;     // [B*T] 1: the frame is a boundary
  int* stage;             // [3][B*T] start, length, kind of the utterance's j-th segment at slot b*T + j
  int* fseg;              // [B*T] the table index of the single-frame segment on this frame, else -1
  int* counts;            // [B] segments of the utterance
  int* urows;             // [B] frames of the utterance that segments own (x_len; 1 when the lengths are out of range)
  int* uflag;             // [B] bit 0: lengths or labels out of range, bit 1: segmented
  double* seg_loss;       // [B*T] loss of every segment
  size_t bytes;
};

inline Work work_layout(void* base, int B, int T) {
  const size_t cap = (size_t)B * (size_t)T;
  unsigned char* p = reinterpret_cast<unsigned char*>(base);
  size_t o = 0;
  Work w;
  w.flags = p + o; o += align_up(cap, 256);
  w.bnd = p + o; o += align_up(cap, 256);
  w.stage = reinterpret_cast<int*>(p + o); o += align_up(3 * cap * sizeof(int), 256);
  w.fseg = reinterpret_cast<int*>(p + o); o += align_up(cap * sizeof(int), 256);
  w.counts = reinterpret_cast<int*>(p + o); o += align_up((size_t)B * sizeof(int), 256);
  w.urows = reinterpret_cast<int*>(p + o); o += align_up((size_t)B * sizeof(int), 256);
  w.uflag = reinterpret_cast<int*>(p + o); o += align_up((size_t)B * sizeof(int), 256);
  w.seg_loss = reinterpret_cast<double*>(p + o); o += align_up(cap * sizeof(double), 256);
  w.bytes = o;
  return w;
}

// the smallest power of two that covers an alphabet row, 64 at the most: lanes per frame
inline int lanes_per_frame(int V) {
  int g = 2;
  while (g < V && g < 64) g <<= 1;
  return g;
}

// ---- plan: match ---------------------------------------------------------------------------------------------------
template <typename IO>
__global__ __launch_bounds__(kThreads) void wordseg_match_kernel(const IO* x, int64_t sB, int64_t sT, int64_t sV,
                                                                 const int64_t* align, const int64_t* x_len,
                                                                 int B, int T, int V, int G, int blank, int space,
                                                                 unsigned char* flags, unsigned char* bnd, int* fseg) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int sub = lane & (G - 1);
  const int64_t R = (int64_t)B * T;
  int64_t row = ((int64_t)blockIdx.x * (kThreads / 64) + wid) * (64 / G) + lane / G;
  const bool live = row < R;
  if (!live) row = R - 1;
  int b, t;
  split_frame(row, T, b, t);
  const int64_t nq = x_len[b];
  const bool act = nq >= 1 && nq <= T && t < (int)nq;
  // (every lane of the wave takes the shuffles below; a frame that is not the utterance's reads nothing)
  const IO* r = x + (int64_t)b * sB + (int64_t)t * sT;
  IO bv = act ? r[0] : (IO)0;
  int bi = 0;
  for (int v = sub; v < (act ? V : 0); v += G) {
    const IO c = r[(int64_t)v * sV];
    if (better(c, v, bv, bi)) { bv = c; bi = v; }
  }
  for (int o = G >> 1; o > 0; o >>= 1) {
    const IO ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if (live && sub == 0) {
    unsigned f = 0;
    if (act) {
      const int64_t a = align[row];
      const bool mis = a != (int64_t)bi;
      const bool sp = !mis && a == (int64_t)space;
      const bool ns = !mis && a != (int64_t)space && a != (int64_t)blank && (t == 0 || align[row - 1] != a);
      f = (mis ? 1u : 0u) | (sp ? 2u : 0u) | (ns ? 4u : 0u);
    }
    flags[row] = (unsigned char)f;
    bnd[row] = 0;
    fseg[row] = -1;
  }
}

// ---- plan: bounds --------------------------------------------------------------------------------------------------
// the automaton between two recognised spaces, folded: `reset` a recognised space lies in the stretch, `m` / `w` mismatches /
// label-run starts behind the last one, `prev` its frame.  join(l, r) = r if r.reset, else (l.reset, l.m + r.m, l.w + r.w, l.prev).
// Exclusive scan of the folds over the workgroup's 256 threads, through LDS (buf: [4][2][kThreads]); identity (0, 0, 0, -1).
__device__ __forceinline__ void block_scan_fold(int& reset, int& m, int& w, int& prev, int* buf) {
  const int tid = threadIdx.x;
  int* br = buf; int* bm = buf + 2 * kThreads; int* bw = buf + 4 * kThreads; int* bp = buf + 6 * kThreads;
  br[tid] = reset; bm[tid] = m; bw[tid] = w; bp[tid] = prev;
  __syncthreads();
  int src = 0;
  for (int o = 1; o < kThreads; o <<= 1) {
    const int c = src * kThreads + tid;
    int r = br[c], mm = bm[c], ww = bw[c], pp = bp[c];
    if (tid >= o && !r) { r = br[c - o]; mm += bm[c - o]; ww += bw[c - o]; pp = bp[c - o]; }
    const int d = (src ^ 1) * kThreads + tid;
    br[d] = r; bm[d] = mm; bw[d] = ww; bp[d] = pp;
    src ^= 1;
    __syncthreads();
  }
  const int c = src * kThreads + tid - 1;
  reset = tid ? br[c] : 0; m = tid ? bm[c] : 0; w = tid ? bw[c] : 0; prev = tid ? bp[c] : -1;
  __syncthreads();
}

__device__ __forceinline__ int block_scan_sum(int v, int* buf /* [2][kThreads] */, int& total) {
  const int tid = threadIdx.x;
  buf[tid] = v;
  __syncthreads();
  int src = 0;
  for (int o = 1; o < kThreads; o <<= 1) {
    int cur = buf[src * kThreads + tid];
    if (tid >= o) cur += buf[src * kThreads + tid - o];
    buf[(src ^ 1) * kThreads + tid] = cur;
    src ^= 1;
    __syncthreads();
  }
  const int res = buf[src * kThreads + tid];
  total = buf[src * kThreads + kThreads - 1];
  __syncthreads();
  return res;
}

__global__ __launch_bounds__(kThreads) void wordseg_bounds_kernel(const int64_t* targets, int64_t tgt_stride,
                                                                  const int64_t* x_len, const int64_t* t_len,
                                                                  int T, int V, int Smax, int min_word_length,
                                                                  const unsigned char* flags_all, unsigned char* bnd_all,
                                                                  int* stage_all, int64_t cap, int* counts, int* urows, int* uflag) {
  __shared__ int fbuf[8 * kThreads];
  __shared__ int ibuf[2 * kThreads];
  __shared__ int first_bound[kThreads];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t base = (int64_t)b * T;
  const unsigned char* flags = flags_all + base;
  unsigned char* bnd = bnd_all + base;
  int* st_start = stage_all + base;
  int* st_len = stage_all + cap + base;
  int* st_kind = stage_all + 2 * cap + base;

  const int64_t nq = x_len[b], sq = t_len[b];
  const bool len_ok = nq >= 1 && nq <= T;
  int bad = !len_ok || sq < 0 || sq > Smax;
  if (!bad) {
    const int64_t* tg = targets + (int64_t)b * tgt_stride;
    for (int j = tid; j < (int)sq; j += kThreads) bad |= (tg[j] < 0) | (tg[j] >= V);
  }
  bad = __syncthreads_or(bad);
  const int n = len_ok ? (int)nq : 1;
  if (bad) {                                  // one whole segment: the loss gives it its NaN slab
    if (tid == 0) { st_start[0] = 0; st_len[0] = n; st_kind[0] = E2E_WORDSEG_WHOLE; counts[b] = 1; urows[b] = n; uflag[b] = 1; }
    return;
  }

  const int per = (n + kThreads - 1) / kThreads;
  const int lo = min(tid * per, n), hi = min(lo + per, n);
  // which spaces qualify
  int f_reset = 0, f_m = 0, f_w = 0, f_prev = -1;
  for (int u = lo; u < hi; u++) {
    const unsigned f = flags[u];
    if (f & 2u) { f_reset = 1; f_m = 0; f_w = 0; f_prev = u; }
    else { f_m += (int)(f & 1u); f_w += (int)((f >> 2) & 1u); }
  }
  block_scan_fold(f_reset, f_m, f_w, f_prev, fbuf);          // now: the state in front of this thread's frames
  for (int u = lo; u < hi; u++) {
    const unsigned f = flags[u];
    if (f & 2u) {
      if (f_m == 0 && f_w >= min_word_length) {
        if (u > 0) bnd[u] = 1;
        if (f_prev >= 0) bnd[f_prev] = 1;
      }
      f_m = 0; f_w = 0; f_prev = u;
    } else { f_m += (int)(f & 1u); f_w += (int)((f >> 2) & 1u); }
  }
  if (tid == 0) { bnd[0] = 1; bnd[n - 1] = 1; }
  // the marks were written by other threads of this workgroup
  __threadfence_block();
  __syncthreads();

  // rank the boundaries
  int nb = 0, fb = 0x7fffffff;
  for (int u = lo; u < hi; u++) if (bnd[u]) { if (!nb) fb = u; nb++; }
  first_bound[tid] = fb;
  int K;
  const int rank0 = block_scan_sum(nb, ibuf, K) - nb;
  if (K <= 2) {
    if (tid == 0) { st_start[0] = 0; st_len[0] = n; st_kind[0] = E2E_WORDSEG_WHOLE; counts[b] = 1; urows[b] = n; uflag[b] = 0; }
    return;
  }
  // the boundary that follows this thread's last one
  int next_after = -1;
  for (int j = tid + 1; j < kThreads && nb; j++) if (first_bound[j] != 0x7fffffff) { next_after = first_bound[j]; break; }

  // boundary k at frame s0 with successor s1: a single-frame segment on s0 unless s0 is frame 0, then the chunk up to the
  // frame before s1 (up to s1 itself for the last pair)
  int off = 0, total = 0;
  for (int pass = 0; pass < 2; pass++) {
    int cnt = 0, k = rank0, pend = -1;
    for (int u = lo; u <= hi; u++) {
      // (u == hi: the boundary that follows the thread's last one, if there is one)
      const int s1 = u < hi ? (bnd[u] ? u : -1) : (pend >= 0 ? next_after : -1);
      if (s1 < 0) continue;
      if (pend >= 0) {
        const int nf = pend != 0 ? 1 : 0;
        const int cs = pend + nf, ce = s1 - (k + 1 == K - 1 ? 0 : 1);
        const int nc = ce >= cs ? 1 : 0;
        if (pass) {
          if (nf) { st_start[off + cnt] = pend; st_len[off + cnt] = 1; st_kind[off + cnt] = E2E_WORDSEG_FRAME; }
          if (nc) { st_start[off + cnt + nf] = cs; st_len[off + cnt + nf] = ce - cs + 1; st_kind[off + cnt + nf] = E2E_WORDSEG_CHUNK; }
        }
        cnt += nf + nc;
        k++;
      }
      pend = s1;
    }
    if (!pass) off = block_scan_sum(cnt, ibuf, total) - cnt;
  }
  if (tid == 0) { counts[b] = total; urows[b] = n; uflag[b] = 2; }
}

// ---- plan: scan ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void wordseg_scan_kernel(const int* counts, int B, int* first /* [B+1] */) {
  __shared__ int ibuf[2 * kThreads];
  const int tid = threadIdx.x;
  const int per = (B + kThreads - 1) / kThreads;
  const int lo = min(tid * per, B), hi = min(lo + per, B);
  int s = 0;
  for (int b = lo; b < hi; b++) s += counts[b];
  int total;
  int run = block_scan_sum(s, ibuf, total) - s;
  for (int b = lo; b < hi; b++) { first[b] = run; run += counts[b]; }
  if (tid == 0) first[B] = total;
}

// ---- plan: table ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void wordseg_table_kernel(const int64_t* align, const int64_t* t_len, int T, int blank,
                                                                 const int* stage_all, int64_t cap, const int* counts,
                                                                 const int* uflag, int* table, int B, int* fseg, int64_t* pool) {
  const int b = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t base = (int64_t)b * T;
  const int* first = table + kHdr;
  int* t_lenf = table + kHdr + (B + 1);
  int* t_tlen = t_lenf + cap;
  int* t_kind = t_tlen + cap;
  int* t_utt = t_kind + cap;
  int* t_start = t_utt + cap;
  const int cnt = counts[b], i0 = first[b];
  for (int j = wid; j < cnt; j += kThreads / 64) {
    const int s = stage_all[base + j], len = stage_all[cap + base + j], kind = stage_all[2 * cap + base + j];
    const int i = i0 + j;
    int tl = 0;
    if (kind == E2E_WORDSEG_WHOLE) tl = (uflag[b] & 1) ? 0 : (int)t_len[b];
    else {
      // the alignment of the frames, runs collapsed, blanks dropped afterwards (a frame segment: its one label, a blank included)
      const int64_t* a = align + base;
      if (kind == E2E_WORDSEG_FRAME) {
        if (lane == 0) { pool[base + s] = a[s]; fseg[base + s] = i; }
        tl = 1;
      } else {
        for (int u0 = 0; u0 < len; u0 += 64) {
          const int u = s + u0 + lane;
          const bool in = u0 + lane < len;
          const int64_t av = in ? a[u] : 0;
          const bool keep = in && av != (int64_t)blank && (u == s || a[u - 1] != av);
          const unsigned long long mask = __ballot(keep);
          if (keep) pool[base + s + tl + __popcll(mask & ((1ull << lane) - 1ull))] = av;
          tl += __popcll(mask);
        }
      }
    }
    if (lane == 0) { t_lenf[i] = len; t_tlen[i] = tl; t_kind[i] = kind; t_utt[i] = b; t_start[i] = s; }
  }
}

// ---- plan: summary -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void wordseg_summary_kernel(int* table, int B, int64_t cap, const int* uflag) {
  __shared__ int acc[8];
  const int tid = threadIdx.x;
  if (tid < 8) acc[tid] = 0;
  __syncthreads();
  const int N = table[kHdr + B];
  const int* t_lenf = table + kHdr + (B + 1);
  const int* t_tlen = t_lenf + cap;
  const int* t_kind = t_tlen + cap;
  int nw = 0, nf = 0, nc = 0, ml = 0, ms = 0, nseg = 0;
  for (int i = tid; i < N; i += 1024) {
    const int k = t_kind[i];
    nw += k == E2E_WORDSEG_WHOLE; nf += k == E2E_WORDSEG_FRAME; nc += k == E2E_WORDSEG_CHUNK;
    if (k != E2E_WORDSEG_FRAME) { ml = max(ml, t_lenf[i]); ms = max(ms, t_tlen[i]); }
  }
  for (int b = tid; b < B; b += 1024) nseg += (uflag[b] >> 1) & 1;
  // (integer sums and maxima: the order in which the lanes arrive does not show)
  atomicAdd(&acc[1], nw); atomicAdd(&acc[2], nf); atomicAdd(&acc[3], nc);
  atomicMax(&acc[4], ml); atomicMax(&acc[5], ms); atomicAdd(&acc[6], nseg);
  __syncthreads();
  if (tid == 0) {
    table[0] = N;
    for (int q = 1; q < 7; q++) table[q] = acc[q];
    for (int q = 7; q < kHdr; q++) table[q] = 0;
  }
}

// ---- gather --------------------------------------------------------------------------------------------------------
template <typename IO>
__global__ __launch_bounds__(kThreads) void wordseg_gather_kernel(const IO* x, int64_t sB, int64_t sT, int64_t sV,
                                                                  const int64_t* targets, int64_t tgt_stride,
                                                                  const int64_t* x_len, const int64_t* t_len,
                                                                  int B, int T, int V, int Smax, const int* table, int64_t cap,
                                                                  const int64_t* pool, const int* idx, int L, int S,
                                                                  IO* xg, int64_t* tg, int64_t* xlg, int64_t* tlg) {
  const int g = blockIdx.x, tid = threadIdx.x;
  const int* t_lenf = table + kHdr + (B + 1);
  const int* t_tlen = t_lenf + cap;
  const int* t_kind = t_tlen + cap;
  const int* t_utt = t_kind + cap;
  const int* t_start = t_utt + cap;
  const int i = idx[g];
  const bool ok = i >= 0 && i < table[0];
  const int b = ok ? t_utt[i] : 0, s = ok ? t_start[i] : 0, kind = ok ? t_kind[i] : E2E_WORDSEG_CHUNK;
  const int len = ok ? min(t_lenf[i], min(L, T - s)) : 0;
  const int tl = ok ? t_tlen[i] : 0;
  const int64_t total = (int64_t)L * V;
  IO* dst = xg + (int64_t)g * total;
  const IO* src = x + (int64_t)b * sB + (int64_t)s * sT;
  const int64_t live = (int64_t)len * V;
  if (sV == 1 && sT == V) {                 // contiguous rows: one flat copy
    for (int64_t e = (int64_t)blockIdx.y * kThreads + tid; e < total; e += (int64_t)gridDim.y * kThreads)
      dst[e] = e < live ? src[e] : (IO)0;
  } else {
    for (int64_t e = (int64_t)blockIdx.y * kThreads + tid; e < total; e += (int64_t)gridDim.y * kThreads) {
      const int t = (int)(e / V), v = (int)(e - (int64_t)t * V);
      dst[e] = e < live ? src[(int64_t)t * sT + (int64_t)v * sV] : (IO)0;
    }
  }
  if (blockIdx.y == 0) {
    const bool whole = kind == E2E_WORDSEG_WHOLE;
    const int64_t tq = whole ? t_len[b] : (int64_t)tl;
    const int ncopy = (int)max((int64_t)0, min(tq, (int64_t)min(S, whole ? Smax : T - s)));
    const int64_t* from = whole ? targets + (int64_t)b * tgt_stride : pool + (int64_t)b * T + s;
    for (int j = tid; j < S; j += kThreads) tg[(int64_t)g * S + j] = j < ncopy ? from[j] : 0;
    // (a whole segment hands the caller's own lengths on: out of range, they stay out of range for the loss)
    if (tid == 0) { xlg[g] = ok ? (whole ? x_len[b] : (int64_t)len) : 0; tlg[g] = ok ? tq : 0; }
  }
}

// ---- finish --------------------------------------------------------------------------------------------------------
template <typename IO>
__global__ __launch_bounds__(kThreads) void wordseg_scatter_kernel(const IO* gg, const IO* gl, const int* idx, int L,
                                                                   const int* table, int B, int64_t cap, int T, int V,
                                                                   double* seg_loss, IO* grads) {
  const int g = blockIdx.x, tid = threadIdx.x;
  const int* t_lenf = table + kHdr + (B + 1);
  const int* t_utt = t_lenf + 3 * cap;
  const int* t_start = t_utt + cap;
  const int i = idx[g];
  if (i < 0 || i >= table[0]) return;
  const int b = t_utt[i], s = t_start[i];
  const int len = min(t_lenf[i], min(L, T - s));
  const int64_t n = (int64_t)len * V;
  const IO* src = gg + (int64_t)g * L * V;
  IO* dst = grads + ((int64_t)b * T + s) * V;            // the segment's frames are consecutive rows of (B,T,V)
  for (int64_t e = (int64_t)blockIdx.y * kThreads + tid; e < n; e += (int64_t)gridDim.y * kThreads) dst[e] = src[e];
  if (blockIdx.y == 0 && tid == 0) seg_loss[i] = (double)gl[g];
}

// the frames no gathered segment owns
template <typename IO>
__global__ __launch_bounds__(kThreads) void wordseg_tail_kernel(const IO* x, int64_t sB, int64_t sT, int64_t sV,
                                                                const int64_t* align, int B, int T, int V, int G,
                                                                const int* table, const int* fseg, const int* urows,
                                                                const int* uflag, double* seg_loss, IO* grads) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int sub = lane & (G - 1);
  const int64_t R = (int64_t)B * T;
  int64_t row = ((int64_t)blockIdx.x * (kThreads / 64) + wid) * (64 / G) + lane / G;
  const bool live = row < R;
  if (!live) row = R - 1;
  int b, t;
  split_frame(row, T, b, t);
  const bool padded = t >= urows[b];
  const int fs = fseg[row];
  const bool act = live && !padded && fs >= 0;
  IO* grow = grads + row * V;
  if (live && padded) {
    // 0 -- or the rest of the NaN slab of an utterance that is one segment whose loss is not finite
    IO fill = (IO)0;
    if (!(uflag[b] & 2)) {
      const double l = seg_loss[table[kHdr + b]];
      if (!(l - l == 0.0)) fill = (IO)__builtin_nan("");
    }
    for (int v = sub; v < V; v += G) grow[v] = fill;
  }
  // a single-frame segment: loss = logsumexp(x_t) - x_t[c], gradient = softmax(x_t) - onehot(c), in f64
  // (every lane of the wave takes the shuffles; the other frames read nothing)
  const IO* r = x + (int64_t)b * sB + (int64_t)t * sT;
  const int Vv = act ? V : 0;
  double m = ninf();
  for (int v = sub; v < Vv; v += G) m = fmax(m, (double)r[(int64_t)v * sV]);
  for (int o = G >> 1; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
  double sum = 0.0;
  for (int v = sub; v < Vv; v += G) sum += exp((double)r[(int64_t)v * sV] - m);
  for (int o = G >> 1; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (act) {
    const double lse = m + log(sum);
    const int c = (int)align[row];
    for (int v = sub; v < V; v += G) grow[v] = (IO)(exp((double)r[(int64_t)v * sV] - lse) - (v == c ? 1.0 : 0.0));
    if (sub == 0) seg_loss[fs] = lse - (double)r[(int64_t)c * sV];
  }
}

template <typename IO>
__global__ __launch_bounds__(kThreads) void wordseg_sum_kernel(const int* table, const double* seg_loss, int B, IO* losses) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= B) return;
  const int* first = table + kHdr;
  double s = 0.0;
  for (int i = first[b]; i < first[b + 1]; i++) s += seg_loss[i];       // table order: two calls agree bit for bit
  losses[b] = (IO)s;
}

bool sizes_ok(int dtype, int B, int T, int V) {
  if (dtype != E2E_F32 && dtype != E2E_F64) { set_error("word segmentation: dtype must be E2E_F32 or E2E_F64"); return false; }
  if (B < 0 || T < 1 || V < 1) { set_error("bad sizes B=%d T=%d V=%d", B, T, V); return false; }
  if ((int64_t)B * T > (int64_t)0x7fffffff / 8) { set_error("word segmentation: B*T = %lld frames are more than the table indexes", (long long)B * T); return false; }
  return true;
}

int tiles_for(int64_t elems) { return (int)max((int64_t)1, min((int64_t)64, (elems + 4 * kThreads - 1) / (4 * kThreads))); }

}  // namespace
}  // namespace e2e

using namespace e2e;

extern "C" size_t e2e_ctc_wordseg_table_elems(int B, int T) {
  if (B < 0 || T < 1 || (int64_t)B * T > (int64_t)0x7fffffff / 8) return 0;
  return (size_t)kHdr + (size_t)B + 1 + 5 * (size_t)B * (size_t)T;
}

extern "C" size_t e2e_ctc_wordseg_workspace_bytes(int B, int T) {
  if (B < 0 || T < 1 || (int64_t)B * T > (int64_t)0x7fffffff / 8) return 0;
  return work_layout(nullptr, B, T).bytes + 256;
}

extern "C" int e2e_ctc_wordseg_plan(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV,
                                    const int64_t* align, const int64_t* targets, int64_t tgt_stride,
                                    const int64_t* x_len, const int64_t* t_len,
                                    int B, int T, int V, int Smax, int blank, int space, int min_word_length,
                                    int32_t* table, size_t table_elems, int64_t* pool,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!sizes_ok(dtype, B, T, V)) return E2E_ERR_ARG;
  if (Smax < 0) { set_error("bad Smax=%d", Smax); return E2E_ERR_ARG; }
  if (blank < 0 || blank >= V) { set_error("blank=%d outside [0,%d)", blank, V); return E2E_ERR_ARG; }
  if (space < 0 || space >= V) { set_error("space=%d outside [0,%d)", space, V); return E2E_ERR_ARG; }
  if (!table || table_elems < e2e_ctc_wordseg_table_elems(B, T)) { set_error("segment table too small: need %zu int32", e2e_ctc_wordseg_table_elems(B, T)); return E2E_ERR_ARG; }
  if (B > 0 && (!x || !align || !x_len || !t_len || !pool || (Smax > 0 && !targets))) { set_error("null pointer argument"); return E2E_ERR_ARG; }
  if (!align_workspace(workspace, workspace_bytes) || workspace_bytes < work_layout(nullptr, B, T).bytes) {
    set_error("workspace too small: need %zu", e2e_ctc_wordseg_workspace_bytes(B, T));
    return E2E_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const Work w = work_layout(workspace, B, T);
  const int64_t cap = (int64_t)B * T;
  if (B > 0) {
    const int G = lanes_per_frame(V);
    const int rows_per_block = (kThreads / 64) * (64 / G);
    const unsigned blocks = (unsigned)((cap + rows_per_block - 1) / rows_per_block);
    if (dtype == E2E_F32)
      hipLaunchKernelGGL(wordseg_match_kernel<float>, dim3(blocks), dim3(kThreads), 0, s, reinterpret_cast<const float*>(x), sB, sT, sV,
                         align, x_len, B, T, V, G, blank, space, w.flags, w.bnd, w.fseg);
    else
      hipLaunchKernelGGL(wordseg_match_kernel<double>, dim3(blocks), dim3(kThreads), 0, s, reinterpret_cast<const double*>(x), sB, sT, sV,
                         align, x_len, B, T, V, G, blank, space, w.flags, w.bnd, w.fseg);
    hipLaunchKernelGGL(wordseg_bounds_kernel, dim3(B), dim3(kThreads), 0, s, targets, tgt_stride, x_len, t_len, T, V, Smax,
                       min_word_length, w.flags, w.bnd, w.stage, cap, w.counts, w.urows, w.uflag);
  }
  hipLaunchKernelGGL(wordseg_scan_kernel, dim3(1), dim3(kThreads), 0, s, w.counts, B, table + kHdr);
  if (B > 0)
    hipLaunchKernelGGL(wordseg_table_kernel, dim3(B), dim3(kThreads), 0, s, align, t_len, T, blank, w.stage, cap, w.counts,
                       w.uflag, table, B, w.fseg, pool);
  hipLaunchKernelGGL(wordseg_summary_kernel, dim3(1), dim3(1024), 0, s, table, B, cap, w.uflag);
  E2E_HIP_CHECK(hipGetLastError(), "word segmentation plan launch");
  return E2E_OK;
}

extern "C" int e2e_ctc_wordseg_gather(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV,
                                      const int64_t* targets, int64_t tgt_stride,
                                      const int64_t* x_len, const int64_t* t_len,
                                      int B, int T, int V, int Smax,
                                      const int32_t* table, const int64_t* pool,
                                      const int32_t* idx, int n_idx, int L, int S,
                                      void* xg, int64_t* tg, int64_t* xlg, int64_t* tlg, void* stream) {
  if (!sizes_ok(dtype, B, T, V)) return E2E_ERR_ARG;
  if (Smax < 0 || n_idx < 0 || L < 1 || L > T || S < 1) { set_error("bad sizes Smax=%d n_idx=%d L=%d S=%d", Smax, n_idx, L, S); return E2E_ERR_ARG; }
  if (n_idx > 0 && (B < 1 || !x || !x_len || !t_len || !table || !pool || !idx || !xg || !tg || !xlg || !tlg || (Smax > 0 && !targets))) {
    set_error("null pointer argument");
    return E2E_ERR_ARG;
  }
  if (n_idx == 0) return E2E_OK;
  hipStream_t s = (hipStream_t)stream;
  const int64_t cap = (int64_t)B * T;
  const dim3 grid((unsigned)n_idx, (unsigned)tiles_for((int64_t)L * V));
  if (dtype == E2E_F32)
    hipLaunchKernelGGL(wordseg_gather_kernel<float>, grid, dim3(kThreads), 0, s, reinterpret_cast<const float*>(x), sB, sT, sV, targets,
                       tgt_stride, x_len, t_len, B, T, V, Smax, table, cap, pool, idx, L, S, reinterpret_cast<float*>(xg), tg, xlg, tlg);
  else
    hipLaunchKernelGGL(wordseg_gather_kernel<double>, grid, dim3(kThreads), 0, s, reinterpret_cast<const double*>(x), sB, sT, sV, targets,
                       tgt_stride, x_len, t_len, B, T, V, Smax, table, cap, pool, idx, L, S, reinterpret_cast<double*>(xg), tg, xlg, tlg);
  E2E_HIP_CHECK(hipGetLastError(), "wordseg_gather_kernel launch");
  return E2E_OK;
}

extern "C" int e2e_ctc_wordseg_finish(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV,
                                      const int64_t* align, int B, int T, int V, const int32_t* table,
                                      const void* g_grads, const void* g_losses, const int32_t* g_idx, int n_idx, int L,
                                      int last, void* losses, void* grads,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  if (!sizes_ok(dtype, B, T, V)) return E2E_ERR_ARG;
  if (n_idx < 0 || (n_idx > 0 && (L < 1 || L > T))) { set_error("bad sizes n_idx=%d L=%d", n_idx, L); return E2E_ERR_ARG; }
  if (B > 0 && (!table || !grads || (n_idx > 0 && (!g_grads || !g_losses || !g_idx)) || (last && (!x || !align || !losses)))) {
    set_error("null pointer argument");
    return E2E_ERR_ARG;
  }
  if (!align_workspace(workspace, workspace_bytes) || workspace_bytes < work_layout(nullptr, B, T).bytes) {
    set_error("workspace too small: need %zu", e2e_ctc_wordseg_workspace_bytes(B, T));
    return E2E_ERR_WORKSPACE;
  }
  if (B == 0) return E2E_OK;
  hipStream_t s = (hipStream_t)stream;
  const Work w = work_layout(workspace, B, T);
  const int64_t cap = (int64_t)B * T;
  if (n_idx > 0) {
    const dim3 grid((unsigned)n_idx, (unsigned)tiles_for((int64_t)L * V));
    if (dtype == E2E_F32)
      hipLaunchKernelGGL(wordseg_scatter_kernel<float>, grid, dim3(kThreads), 0, s, reinterpret_cast<const float*>(g_grads),
                         reinterpret_cast<const float*>(g_losses), g_idx, L, table, B, cap, T, V, w.seg_loss, reinterpret_cast<float*>(grads));
    else
      hipLaunchKernelGGL(wordseg_scatter_kernel<double>, grid, dim3(kThreads), 0, s, reinterpret_cast<const double*>(g_grads),
                         reinterpret_cast<const double*>(g_losses), g_idx, L, table, B, cap, T, V, w.seg_loss, reinterpret_cast<double*>(grads));
  }
  if (last) {
    const int G = lanes_per_frame(V);
    const int rows_per_block = (kThreads / 64) * (64 / G);
    const unsigned blocks = (unsigned)((cap + rows_per_block - 1) / rows_per_block);
    const unsigned ublocks = (unsigned)((B + kThreads - 1) / kThreads);
    if (dtype == E2E_F32) {
      hipLaunchKernelGGL(wordseg_tail_kernel<float>, dim3(blocks), dim3(kThreads), 0, s, reinterpret_cast<const float*>(x), sB, sT, sV, align,
                         B, T, V, G, table, w.fseg, w.urows, w.uflag, w.seg_loss, reinterpret_cast<float*>(grads));
      hipLaunchKernelGGL(wordseg_sum_kernel<float>, dim3(ublocks), dim3(kThreads), 0, s, table, w.seg_loss, B, reinterpret_cast<float*>(losses));
    } else {
      hipLaunchKernelGGL(wordseg_tail_kernel<double>, dim3(blocks), dim3(kThreads), 0, s, reinterpret_cast<const double*>(x), sB, sT, sV, align,
                         B, T, V, G, table, w.fseg, w.urows, w.uflag, w.seg_loss, reinterpret_cast<double*>(grads));
      hipLaunchKernelGGL(wordseg_sum_kernel<double>, dim3(ublocks), dim3(kThreads), 0, s, table, w.seg_loss, B, reinterpret_cast<double*>(losses));
    }
  }
  E2E_HIP_CHECK(hipGetLastError(), "word segmentation finish launch");
  return E2E_OK;
}
