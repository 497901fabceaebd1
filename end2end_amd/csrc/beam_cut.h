// The per-frame cut of the n-best prefix beam searches that keep their members in LDS (ctc_gram_decode.hip, asg_beam.hip):
// of a frame's candidates the W with the largest totals survive, exactly equal totals by ascending 64-bit prefix key, and
// the survivors are ranked in that order.  Device only; one workgroup per utterance calls it, all threads.
//
// A caller hands over the candidates that passed its own filter as sval[0 .. nsv): the totals in an encoding whose
// unsigned order and equality are the totals' own (what the encoding is, and what the filter drops, is the caller's), and
// spos[0 .. nsv): whatever the caller needs to find a candidate again.  The select compares encoded bits only; a survivor's
// total is decoded once, by the caller's total_of, and the ranking compares the numbers (ranking on the bits instead
// measured 0.2 % slower per call at width 100).
#pragma once
#include "common.h"

namespace e2e {

// a prefix's key: FNV-1a over its ids from kKeyBasis (0 marks a free table entry: a key of 0 is stored as 1); a key's
// home slot in a table of 2^n entries: (key * kHashMul) >> (64 - n)
constexpr uint64_t kKeyBasis = 0xcbf29ce484222325ull, kKeyPrime = 0x100000001b3ull;
constexpr uint64_t kHashMul = 0x9e3779b97f4a7c15ull;

constexpr int kMaxW = 128;                 // members of a beam (LDS)

// The encoding of a total that the beam searches hand to a select (here, and the radix select of ctc_beam_common.h): an
// order-preserving map double -> uint64, larger double <=> larger key.  -0.0 and +0.0 compare equal as doubles -- the oracle's
// order -- so the key is taken of d + 0.0, which is +0.0 for both.
__device__ __forceinline__ unsigned long long okey(double d) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(d + 0.0);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// a streaming search's member set between LDS and its state row, as it stands: `bytes` (a multiple of 8) copied by all
// kThreads threads of the workgroup in plain vector loads and stores
template <int kThreads>
__device__ __forceinline__ void stream_copy(void* dst, const void* src, size_t bytes) {
  const unsigned long long* s = reinterpret_cast<const unsigned long long*>(src);
  unsigned long long* d = reinterpret_cast<unsigned long long*>(dst);
  for (size_t i = threadIdx.x; i < bytes / 8; i += kThreads) d[i] = s[i];
}

// the cut's LDS state: a kernel declares one __shared__ and zeroes n_sel (behind a barrier) before every beam_cut
struct BeamCut {
  double sel_tot[kMaxW];                                // the survivors: total,
  unsigned long long sel_key[kMaxW];                    // key,
  int sel_pos[kMaxW], sel_rank[kMaxW];                  // the caller's spos, and (beam_cut_rank) the rank
  unsigned hist[256];
  int n_sel, digit, need, count;
  int wave_part[4];
};

// Selects among sval[0 .. nsv) and gathers the survivors into S.sel_pos / sel_tot / sel_key in any order; S.n_sel counts
// them.  key_of(pos) is the 64-bit key of the candidate whose spos is pos, total_of(bits) the total encoded as bits.
// Begins behind the barrier that completes sval / spos and ends WITHOUT one: the caller's barrier follows, then
// beam_cut_count.  The barriers inside are one per phase of a pass: the digit of pass k is read by every thread before
// thread 0 resets it behind the first barrier of pass k + 1.
template <int kThreads, typename KeyOf, typename TotalOf>
__device__ __forceinline__ void beam_cut(BeamCut& S, const unsigned long long* sval, const int* spos, int nsv, int W,
                                         KeyOf key_of, TotalOf total_of) {
  static_assert(kThreads >= 256 && kThreads % 64 == 0, "the digit search runs on threads 0 .. 255, four whole waves");
  const int tid = threadIdx.x;
  unsigned long long thr = 0ull, kthr = ~0ull;                   // selected: bits > thr, or bits == thr and key <= kthr
  if (nsv > W) {
    int need = W;
    for (int shift = 56; shift >= 0; shift -= 8) {
      if (tid < 256) S.hist[tid] = 0u;
      __syncthreads();
      if (tid == 0) { S.digit = 0; S.need = need; S.count = 0; }   // (behind the barrier: the last pass' digit has been read)
      const unsigned long long mask = shift == 56 ? 0ull : (~0ull << (shift + 8));
      for (int i = tid; i < nsv; i += kThreads) {
        const unsigned long long v = sval[i];
        if ((v & mask) == thr) atomicAdd(&S.hist[(unsigned)(v >> shift) & 255u], 1u);
      }
      __syncthreads();
      // the digit: the bin d with (count above d) < need <= (count above d) + hist[d]; a suffix sum over 256 threads
      int h = 0, incl = 0;
      if (tid < 256) {
        h = (int)S.hist[tid]; incl = h;
        for (int o = 1; o < 64; o <<= 1) { const int n = __shfl_down(incl, o, 64); if ((tid & 63) + o < 64) incl += n; }
        if ((tid & 63) == 0) S.wave_part[tid >> 6] = incl;
      }
      __syncthreads();
      if (tid < 256) {
        int above = incl - h;
        for (int w = (tid >> 6) + 1; w < 4; w++) above += S.wave_part[w];
        if (h > 0 && above < need && need <= above + h) { S.digit = tid; S.need = need - above; S.count = h; }
      }
      __syncthreads();
      thr |= (unsigned long long)S.digit << shift;
      need = S.need;
    }
    if (S.count > need) {                                        // more equal totals than places: the `need` smallest keys
      unsigned long long kpre = 0ull;
      for (int shift = 56; shift >= 0; shift -= 8) {
        __syncthreads();
        if (tid < 256) S.hist[tid] = 0u;
        if (tid == 0) { S.digit = 255; S.need = need; }
        __syncthreads();
        const unsigned long long mask = shift == 56 ? 0ull : (~0ull << (shift + 8));
        for (int i = tid; i < nsv; i += kThreads) {
          if (sval[i] != thr) continue;
          const unsigned long long kk = key_of(spos[i]);
          if ((kk & mask) == kpre) atomicAdd(&S.hist[(unsigned)(kk >> shift) & 255u], 1u);
        }
        __syncthreads();
        int h = 0, incl = 0;
        if (tid < 256) {
          h = (int)S.hist[tid]; incl = h;
          for (int o = 1; o < 64; o <<= 1) { const int n = __shfl_up(incl, o, 64); if ((tid & 63) >= o) incl += n; }
          if ((tid & 63) == 63) S.wave_part[tid >> 6] = incl;
        }
        __syncthreads();
        if (tid < 256) {
          int below = incl - h;
          for (int w = 0; w < (tid >> 6); w++) below += S.wave_part[w];
          if (h > 0 && below < need && need <= below + h) { S.digit = tid; S.need = need - below; }
        }
        __syncthreads();
        kpre |= (unsigned long long)S.digit << shift;
        need = S.need;
      }
      kthr = kpre;
    }
  }
  __syncthreads();
  for (int i = tid; i < nsv; i += kThreads) {
    const unsigned long long v = sval[i];
    if (v < thr) continue;
    const int pos = spos[i];
    const unsigned long long kk = key_of(pos);
    if (v == thr && kk > kthr) continue;
    const int j = atomicAdd(&S.n_sel, 1);
    if (j < W) { S.sel_pos[j] = pos; S.sel_tot[j] = total_of(v); S.sel_key[j] = kk; }
  }
}

// the number of survivors gathered; behind the barrier that follows beam_cut
__device__ __forceinline__ int beam_cut_count(const BeamCut& S, int W) { return min(S.n_sel, W); }

// S.sel_rank[i] of survivor i < ns: how many survivors precede it (total descending, key ascending); two survivors with
// one total and one key (2^-64) share a rank, and no rank leaves [0, ns).  No barrier: a thread may read its own rank at
// once, another's behind the caller's.
__device__ __forceinline__ void beam_cut_rank(BeamCut& S, int ns) {
  const int tid = threadIdx.x;
  if (tid < ns) {
    const double mt = S.sel_tot[tid]; const unsigned long long mk = S.sel_key[tid];
    int r = 0;
    for (int i = 0; i < ns; i++) r += (S.sel_tot[i] > mt || (S.sel_tot[i] == mt && S.sel_key[i] < mk)) ? 1 : 0;
    if (r >= ns) r = ns - 1;
    S.sel_rank[tid] = r;
  }
}

}  // namespace e2e
