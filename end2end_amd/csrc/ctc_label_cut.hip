// Per-frame label pruning (cutoff_top_n, cutoff_prob): which labels of a frame a pruned beam search expands.
// The definition is in include/e2e_ctc.h (e2e_ctc_label_cut), the account of the kernel in DESIGN.md 4.4.
//
// A frame is independent of every other, so the selection is a kernel of its own over the B*T frames, not a phase of the
// one-workgroup-per-utterance search that is serial in t.  One GROUP of threads takes one frame: a wave (four frames per
// 256-thread workgroup, no workgroup barrier at all) for rows of up to kWaveMaxV columns, a 256-thread workgroup beyond.
//   1. the row is read once, coalesced along V, into LDS as order-preserving integer keys (rows of up to kStageBytes; a
//      longer row is read again from L2 / HBM by every pass below);
//   2. radix select of the K-th largest (key descending, id ascending), 8 bits per pass on integer histograms in LDS: the
//      passes over the key's bits stop at the first whose threshold bin survives whole; only a threshold bin with more
//      equal keys than places goes on over the bits of the id;
//   3. the K winners are gathered (in any order: an integer counter in LDS) and ranked by counting;
//   4. cutoff_prob < 1: exp() of the winners in rank order, a fixed-shape (Hillis-Steele) f64 scan in LDS, the first place
//      whose sum reaches cutoff_prob; cutoff_prob == 1 skips 3's ranking and this step;
//   5. the kept winners and the blank are placed in ascending id by counting, -1 behind them (without a blank -- the ASG
//      search's lists, BLANK = false -- the K winners alone, stride K).
// No floating-point atomics: the f64 sums are a scan of fixed shape over a fixed order, so a call repeats bit for bit.
#include "ctc_beam_common.h"

namespace e2e {
namespace beamk {
namespace {

constexpr int kCutThreads = 256;
constexpr int kCutMaxK = 1024;                 // e2e_ctc_label_cut_max()
constexpr int kWaveMaxV = 256;                 // a wave per frame up to here (and K <= V)
constexpr int kStageBytes = 32 * 1024;         // a row's keys in LDS: 8192 columns of f32 / 16-bit, 4096 of f64

// The order-preserving key of a log-probability as the search reads it: f32 / 16-bit inputs as their f32 image, f64 as it is.
// NaN counts as -inf; -0 and +0 are one number (x + 0).  `value` is the inverse, exact.
template <typename IO> struct CutKey {
  typedef unsigned T;
  static constexpr int kBits = 32;
  __device__ static T key(IO x) {
    float f = (float)x;
    if (f != f) f = -INFINITY;
    const unsigned u = __float_as_uint(f + 0.f);
    return (u >> 31) ? ~u : (u | 0x80000000u);
  }
  __device__ static double value(T k) { return (double)__uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }
};
template <> struct CutKey<double> {
  typedef unsigned long long T;
  static constexpr int kBits = 64;
  __device__ static T key(double d) {
    if (d != d) d = -__builtin_huge_val();
    const unsigned long long u = (unsigned long long)__double_as_longlong(d + 0.0);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
  }
  __device__ static double value(T k) { return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k)); }
};

struct CutParams {
  const void* lp; int64_t sB, sT, sV; const int64_t* x_len;
  int B, T, V, blank, K;                       // K = min(cutoff_top_n, V)
  double prob;                                 // cutoff_prob
  int* ids; int* n;                            // (B,T,K+1), (B,T)
  int staged;                                  // the row's keys are kept in LDS
  int group_bytes;                             // LDS of one group
};

// LDS of one group (a frame): [keys: V, when staged] [winners' keys: K] [P0, P1: K doubles each] [hist: 256] [winners' ids:
// K + 1] [ranks: K + 1] [scalars: 16], the 8-byte types first
__host__ __device__ inline size_t cut_group_bytes(int V, int K, int key_bytes, bool staged) {
  size_t o = staged ? ((size_t)V * key_bytes + 7) / 8 * 8 : 0;
  o += ((size_t)K * key_bytes + 7) / 8 * 8;
  o += 2 * sizeof(double) * (size_t)K;
  o += sizeof(int) * (256 + 2 * ((size_t)K + 1) + 16);
  return (o + 15) / 16 * 16;
}

// the barrier of a group: a wave's LDS accesses complete in order, so a wave only has to wait for them; a workgroup meets
template <int G> __device__ __forceinline__ void cut_sync() {
  if (G == 64) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  else __syncthreads();
}

// BLANK = false (the ASG search's lists: there is no blank, and cutoff_prob is 1): step 5 adds nothing, a frame's list is
// its K winners in ascending id with stride K, and its count is K.
template <typename IO, int G, bool BLANK = true>
__global__ __launch_bounds__(kCutThreads) void label_cut_kernel(CutParams p) {
  constexpr int kPad = BLANK ? 1 : 0;
  typedef CutKey<IO> KF;
  typedef typename KF::T KeyT;
  extern __shared__ __align__(16) unsigned char cut_smem[];
  const int tid = threadIdx.x, gt = tid % G, grp = tid / G, lane = tid & 63;
  const int64_t frame = (int64_t)blockIdx.x * (kCutThreads / G) + grp;
  if (frame >= (int64_t)p.B * p.T) return;                       // (a whole group: a wave, or the workgroup)
  int b, t;
  split_frame(frame, p.T, b, t);
  const int64_t xl = p.x_len[b];
  if (t >= xl) { if (gt == 0) p.n[frame] = 0; return; }
  const int V = p.V, K = p.K, blank = p.blank;
  const IO* const row = reinterpret_cast<const IO*>(p.lp) + (int64_t)b * p.sB + (int64_t)t * p.sT;

  unsigned char* q8 = cut_smem + (size_t)grp * p.group_bytes;
  KeyT* const keys = (KeyT*)q8; if (p.staged) q8 += ((size_t)V * sizeof(KeyT) + 7) / 8 * 8;
  KeyT* const wk = (KeyT*)q8; q8 += ((size_t)K * sizeof(KeyT) + 7) / 8 * 8;
  double* P0 = (double*)q8; q8 += sizeof(double) * (size_t)K;
  double* P1 = (double*)q8; q8 += sizeof(double) * (size_t)K;
  int* const hist = (int*)q8; q8 += sizeof(int) * 256;
  int* const wi = (int*)q8; q8 += sizeof(int) * ((size_t)K + 1);
  int* const rk = (int*)q8; q8 += sizeof(int) * ((size_t)K + 1);
  int* const sc = (int*)q8;                                      // [0] digit [1] rest [2] count [3] winners [4] k [5] blank kept [8..] wave sums
  const bool staged = p.staged != 0;
  const int64_t sV = p.sV;
  const double prob = p.prob;
  auto KEY = [&](int c) -> KeyT { return staged ? keys[c] : KF::key(row[(int64_t)c * sV]); };

  if (staged) for (int c = gt; c < V; c += G) keys[c] = KF::key(row[(int64_t)c * sV]);
  if (gt == 0) { sc[3] = 0; sc[4] = K; sc[5] = 0; }
  cut_sync<G>();

  // One pass of a radix select: the histogram of digit(c) over the columns that are still in, then the digit at which the
  // count from the top reaches `want`.  Leaves sc[0] the digit, sc[1] how many of its sc[2] columns are still wanted.
  constexpr int kPer = 256 / G;
  auto select_pass = [&](int want, auto digit_of) {
    for (int h = gt; h < 256; h += G) hist[h] = 0;
    cut_sync<G>();
    for (int c = gt; c < V; c += G) { const int d = digit_of(c); if (d >= 0) atomicAdd(&hist[d], 1); }
    cut_sync<G>();
    int cnt[kPer], mine = 0;
    const int top = 255 - kPer * gt;                             // this thread's bins, the largest digit first
#pragma unroll
    for (int jj = 0; jj < kPer; jj++) { cnt[jj] = hist[top - jj]; mine += cnt[jj]; }
    const int inc = wave_scan_i(mine);
    int above = inc - mine;
    if (G > 64) {
      if (lane == 63) sc[8 + (gt >> 6)] = inc;
      cut_sync<G>();
      for (int w2 = 0; w2 < (gt >> 6); w2++) above += sc[8 + w2];
    }
    if (above < want && above + mine >= want) {
#pragma unroll
      for (int jj = 0; jj < kPer; jj++) {
        if (above + cnt[jj] >= want) { sc[0] = top - jj; sc[1] = want - above; sc[2] = cnt[jj]; break; }
        above += cnt[jj];
      }
    }
    cut_sync<G>();
  };

  // ---- the K-th place: vthr under vmask, and among the columns that equal it the ids up to idmax ----
  KeyT vthr = 0, vmask = 0;
  int idmax = 0x7fffffff;
  if (K < V) {
    int want = K;
    bool whole = false;
    for (int shift = KF::kBits - 8; shift >= 0 && !whole; shift -= 8) {
      const KeyT pre = vthr, msk = vmask;
      select_pass(want, [&](int c) -> int { const KeyT u = KEY(c); return (u & msk) == pre ? (int)((u >> shift) & 0xff) : -1; });
      vthr |= (KeyT)sc[0] << shift; vmask |= (KeyT)0xff << shift;
      want = sc[1]; whole = sc[2] == want;
      cut_sync<G>();                                             // (sc[] is read before the next pass writes it)
    }
    if (!whole) {
      // more equal keys than places: the `want` smallest ids among them (the inverted id's largest, by the same passes)
      int nb = 1; while (nb < 4 && ((unsigned)(V - 1) >> (8 * nb)) != 0u) nb++;
      const unsigned full = nb == 4 ? 0xffffffffu : ((1u << (8 * nb)) - 1u);
      unsigned ithr = 0u, imask = 0u;
      for (int shift = 8 * (nb - 1); shift >= 0; shift -= 8) {
        const unsigned pre = ithr, msk = imask;
        select_pass(want, [&](int c) -> int {
          if (KEY(c) != vthr) return -1;
          const unsigned ic = ~(unsigned)c & full;
          return (ic & msk) == pre ? (int)((ic >> shift) & 0xffu) : -1;
        });
        ithr |= (unsigned)sc[0] << shift; imask |= 0xffu << shift;
        want = sc[1];
        cut_sync<G>();
      }
      idmax = (int)(~ithr & full);
    }
  }
  // ---- the winners, in any order ----
  for (int c = gt; c < V; c += G) {
    const KeyT u = KEY(c), um = u & vmask;
    if (um > vthr || (um == vthr && c <= idmax)) {
      const int j = atomicAdd(&sc[3], 1);
      if (j < K) { wk[j] = u; wi[j] = c; }
    }
  }
  cut_sync<G>();
  // ---- cutoff_prob: rank, scan, the first place that reaches it ----
  int k = K;
  if (prob < 1.0) {
    for (int e = gt; e < K; e += G) {
      const KeyT ke = wk[e]; const int ie = wi[e];
      int r = 0;
      for (int j = 0; j < K; j++) { const KeyT kj = wk[j]; r += (kj > ke || (kj == ke && wi[j] < ie)) ? 1 : 0; }
      rk[e] = r;
      P0[r] = exp(KF::value(ke));                                // (the ranks are a permutation of 0 .. K-1)
    }
    cut_sync<G>();
    for (int off = 1; off < K; off <<= 1) {
      for (int r = gt; r < K; r += G) P1[r] = r >= off ? P0[r - off] + P0[r] : P0[r];
      cut_sync<G>();
      double* const sw = P0; P0 = P1; P1 = sw;
    }
    for (int r = gt; r < K; r += G) if (P0[r] >= prob) atomicMin(&sc[4], r + 1);
    cut_sync<G>();
    k = sc[4];
  } else {
    for (int e = gt; e < K; e += G) rk[e] = 0;
  }
  // ---- the kept set in ascending id, the blank always among them ----
  int extra = 0;
  if constexpr (BLANK) {
    for (int e = gt; e < K; e += G) if (rk[e] < k && wi[e] == blank) sc[5] = 1;
    cut_sync<G>();
    extra = sc[5] ? 0 : 1;
    if (extra && gt == 0) { wi[K] = blank; rk[K] = -1; }
    cut_sync<G>();
  } else {
    cut_sync<G>();                                               // (the ranks are read below)
  }
  const int nw = K + extra, nout = k + extra;
  int* const out = p.ids + frame * ((int64_t)K + kPad);
  for (int e = gt; e < nw; e += G) {
    if (rk[e] >= k) continue;
    const int ie = wi[e];
    int pos = 0;
    for (int j = 0; j < nw; j++) pos += (rk[j] < k && wi[j] < ie) ? 1 : 0;
    if (pos < K + kPad) out[pos] = ie;
  }
  for (int e = nout + gt; e < K + kPad; e += G) out[e] = -1;
  if (gt == 0) p.n[frame] = nout;
}

template <typename IO, bool BLANK = true>
int launch_cut_of(const CutParams& p0, hipStream_t s) {
  CutParams p = p0;
  typedef typename CutKey<IO>::T KeyT;
  const bool wave = p.V <= kWaveMaxV;
  if (!BLANK && !wave) { set_error("a selection without a blank: V=%d, at most %d", p.V, kWaveMaxV); return E2E_ERR_UNSUPPORTED; }
  p.staged = (size_t)p.V * sizeof(KeyT) <= (size_t)kStageBytes ? 1 : 0;
  p.group_bytes = (int)cut_group_bytes(p.V, p.K, (int)sizeof(KeyT), p.staged != 0);
  const int per = wave ? kCutThreads / 64 : 1;
  const size_t lds = (size_t)p.group_bytes * per;
  const int64_t frames = (int64_t)p.B * p.T;
  const int64_t blocks = (frames + per - 1) / per;
  const void* fn = !BLANK ? reinterpret_cast<const void*>(&label_cut_kernel<IO, 64, BLANK>)   // (only the wave form is built)
                 : wave ? reinterpret_cast<const void*>(&label_cut_kernel<IO, 64>)
                        : reinterpret_cast<const void*>(&label_cut_kernel<IO, kCutThreads>);
  E2E_HIP_CHECK(allow_dynamic_lds(fn, (int)lds), "hipFuncSetAttribute");
  void* args[] = { &p };
  E2E_HIP_CHECK(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(kCutThreads), args, lds, s), "label_cut_kernel launch");
  E2E_HIP_CHECK(hipGetLastError(), "label_cut_kernel launch");
  return E2E_OK;
}

}  // namespace

int label_cut_check(int dtype, int B, int T, int V, int blank, int cutoff_top_n, double cutoff_prob) {
  if (dtype != E2E_F32 && dtype != E2E_F64 && !dtype_is_16bit(dtype)) { set_error("dtype must be E2E_F32, E2E_F64, E2E_F16 or E2E_BF16"); return E2E_ERR_ARG; }
  if (B < 0 || T < 1 || V < 1) { set_error("bad sizes"); return E2E_ERR_ARG; }
  if (blank < 0 || blank >= V) { set_error("blank=%d outside [0,%d)", blank, V); return E2E_ERR_ARG; }
  if (cutoff_top_n < 1) { set_error("cutoff_top_n=%d: at least 1", cutoff_top_n); return E2E_ERR_ARG; }
  if (!(cutoff_prob > 0.0 && cutoff_prob <= 1.0)) { set_error("cutoff_prob=%g outside (0, 1]", cutoff_prob); return E2E_ERR_ARG; }
  if ((int64_t)B * T > 0x7fffffffLL / 2) { set_error("bad sizes: B*T"); return E2E_ERR_ARG; }
  if (label_cut_k(V, cutoff_top_n) > kCutMaxK) {
    set_error("min(cutoff_top_n, V) = %d: at most %d labels of a frame can be kept", label_cut_k(V, cutoff_top_n), kCutMaxK);
    return E2E_ERR_UNSUPPORTED;
  }
  return E2E_OK;
}

int launch_label_cut(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len, int B, int T, int V,
                     int blank, int cutoff_top_n, double cutoff_prob, int* ids, int* n, hipStream_t s) {
  CutParams p;
  p.lp = lp; p.sB = sB; p.sT = sT; p.sV = sV; p.x_len = x_len;
  p.B = B; p.T = T; p.V = V; p.blank = blank; p.K = label_cut_k(V, cutoff_top_n);
  p.prob = cutoff_prob; p.ids = ids; p.n = n; p.staged = 0; p.group_bytes = 0;
  if (blank < 0) {                                               // no blank (the ASG search): ids (B,T,K), cutoff_prob 1, f32 / f64
    if (cutoff_prob != 1.0 || (dtype != E2E_F32 && dtype != E2E_F64)) { set_error("a selection without a blank: f32 / f64, cutoff_prob 1"); return E2E_ERR_ARG; }
    return dtype == E2E_F32 ? launch_cut_of<float, false>(p, s) : launch_cut_of<double, false>(p, s);
  }
  switch (dtype) {
    case E2E_F32: return launch_cut_of<float>(p, s);
    case E2E_F64: return launch_cut_of<double>(p, s);
    case E2E_F16: return launch_cut_of<f16_t>(p, s);
    default:      return launch_cut_of<bf16_t>(p, s);
  }
}

}  // namespace beamk
}  // namespace e2e

using namespace e2e;
using namespace e2e::beamk;

extern "C" int e2e_ctc_label_cut_max(void) { return kCutMaxK; }

// (the selection lives in LDS: the workspace is a token block, so that callers size and pass it like every other call's)
extern "C" size_t e2e_ctc_label_cut_workspace_bytes(int B, int T, int V, int cutoff_top_n) {
  if (B < 0 || T < 1 || V < 1 || cutoff_top_n < 1) return 0;
  return 256;
}

extern "C" int e2e_ctc_label_cut(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len,
                                 int B, int T, int V, int blank, int cutoff_top_n, double cutoff_prob,
                                 int32_t* ids, int32_t* n, void* workspace, size_t workspace_bytes, void* stream) {
  (void)workspace; (void)workspace_bytes;
  if (const int rc = label_cut_check(dtype, B, T, V, blank, cutoff_top_n, cutoff_prob)) return rc;
  if (B > 0 && (!lp || !x_len || !ids || !n)) { set_error("null pointer argument"); return E2E_ERR_ARG; }
  if (B == 0) return E2E_OK;
  return launch_label_cut(lp, dtype, sB, sT, sV, x_len, B, T, V, blank, cutoff_top_n, cutoff_prob, ids, n, (hipStream_t)stream);
}
