// The Gram-CTC beam search's device code and the host-side helpers its translation units share: ctc_gram_decode.hip (the
// unpruned instances, where the account of the search is) and ctc_gram_decode_cut.hip (the pruned ones, CUT).
#pragma once
#include <cstddef>
#include <cstring>
#include <initializer_list>
#include <type_traits>

#include "beam_cut.h"
#include "ctc_lm.h"

namespace e2e {
namespace {

constexpr int kBeamThreads = 1024;
constexpr int kMaxK = 8;                   // longest gram
constexpr int kMaxPairs = 131072;          // beam_width * V

__device__ __forceinline__ int order_of(const int32_t* gram_len, int c, int K) {
  const int k = gram_len[c];
  return k < 1 ? 1 : (k > K ? K : k);
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

// ---- the pruned search (CUT, ctc_gram_decode_cut.hip): a frame's kept columns, kept[0 .. n), ascending, kept[0] the blank ----
// A pair's id is m * S + j, S = K_cut + 1 the list's stride and j the place of its column in the list; j == 0: member m
// itself.  y[j] is the probability of column kept[j].  Nodes and members keep real columns, so j is translated back here.
// the column at place j; a place that holds no column of the table (never one the selection wrote) reads as the blank
__device__ __forceinline__ int kept_col(const int32_t* kept, int j, int V) {
  const int c = j > 0 ? kept[j] : 0;
  return (unsigned)c < (unsigned)V ? c : 0;
}
// the place of column c >= 1 in the list, or -1: the column is not kept and does nothing in this frame
__device__ __forceinline__ int kept_find(const int32_t* kept, int n, int c) {
  int lo = 1, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (kept[mid] < c) lo = mid + 1; else hi = mid;
  }
  return (lo < n && kept[lo] == c) ? lo : -1;
}
// eval_list over the kept columns: a slot whose column is not kept has no "run continues" share in this frame
__device__ __forceinline__ void eval_list_cut(Eval& E, const Members& M, int head, const int* next, const double* y,
                                              const int32_t* kept, int n, const int32_t* gram_len, unsigned S, int V, int K,
                                              unsigned n_ids) {
#pragma unroll
  for (int k = 0; k <= kMaxK; k++) { E.s[k] = 0.0; E.c[k] = 0; }
  E.stay = -1; E.pair = 0x7fffffff;
  int id = head;
  for (int steps = 0; steps < 2 * (kMaxK + 1) && (unsigned)id < n_ids; steps++) {
    const unsigned m = (unsigned)id / S, j = (unsigned)id - m * S;
    if (j == 0) {
      E.stay = (int)m;
      E.s[0] += M.tot[m] * y[0];
#pragma unroll
      for (int k = 1; k <= kMaxK; k++)
        if (k <= K) {
          const double pk = M.p[k][m];
          if (pk > 0.0) {
            const int ck = M.col[k][m];
            const int jk = kept_find(kept, n, ck);
            if (jk > 0) { E.s[k] += pk * y[jk]; if (!E.c[k]) E.c[k] = ck; }
          }
        }
    } else {
      const int c = kept_col(kept, (int)j, V);
      const int k = order_of(gram_len, c, K);
      const double v = ext_source(M, (int)m, k, c, K) * y[j];
#pragma unroll
      for (int kk = 1; kk <= kMaxK; kk++) if (kk == k) { E.s[kk] += v; E.c[kk] = c; }
      if (id < E.pair) E.pair = id;
    }
    id = next[id];
  }
}
// a candidate's slots, by the instance's walk
template <bool CUT>
__device__ __forceinline__ void eval_cand(Eval& E, const Members& M, int head, const int* next, const double* y,
                                          const int32_t* kept, int n_kept, const int32_t* gram_len, unsigned S, int V, int K,
                                          unsigned n_ids) {
  if constexpr (CUT) eval_list_cut(E, M, head, next, y, kept, n_kept, gram_len, S, V, K, n_ids);
  else eval_list(E, M, head, next, y, gram_len, (unsigned)V, K, n_ids);
}

// ---- the language model's part (the LM instance only) ---------------------------------------------------------------
constexpr unsigned long long kNoCand = 0ull;   // okey() of nothing: below every number's key (okey(-inf) = 0x000f...f)
__device__ __forceinline__ double okey_inv(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}

// the LM fields of a member: asg_beam.hip's LmMembers, and with them the number of words, the last base id (-1: the empty
// prefix) and the row of the answer cache that holds the member's children
struct LmMembers {
  unsigned long long hash[kMaxW];        // running FNV hash of the last word's spelling
  double lm[kMaxW], lmb[kMaxW];          // lm_score, lm_before
  int oov[kMaxW], oovb[kMaxW];
  unsigned st[kCtx][kMaxW], stb[kCtx][kMaxW];   // LM context after / before the last word, most recent first
  int stn[kMaxW], stbn[kMaxW];
  int nw[kMaxW], last[kMaxW], row[kMaxW];
};
// the LM instance's LDS: both member sets' fields and the frame's row bookkeeping (rows < 2 * kMaxW = 256, ranks < kMaxW)
struct LmState {
  LmMembers lms[2];
  unsigned char used[2 * kMaxW];         // the row belongs to a member that stays
  unsigned char free_list[2 * kMaxW];
  unsigned char new_list[kMaxW];         // the ranks of the frame's new members
  int n_stay, n_new, n_free;
};
struct Answer { double lm; int nw, oov; };                       // what the cut needs of a child: 16 bytes per (row, column)
constexpr int kNoChild = -1;                                     // Answer::nw of a child that a restricted search does not form

struct GramLmParams {
  GramBeamParams b;
  LmView lm; int has_lm, space_id, R; double lmwt, wip, oov;    // R: the base labels, the model's label strings
  int32_t* counts; size_t off_cache;
};
// the parameter block of the instances of e2e_gram_ctc_beam_nbest_opt (LEX or TS): the LM instance's and what it lacks.  A
// block of its own, so that the two instances that were there before keep theirs, and with it their code.
struct GramOptParams { GramLmParams l; int64_t* timesteps; };   // (B,nbest,max_out): the TS instances only

// ---- the state row of a stream (e2e_gram_ctc_beam_stream): header (256 bytes) | Members | LmMembers (scored) | node pool ----
// Indices only, never an address: a row may be moved or copied.  magic == 0 -- what a zeroed header has -- is a fresh utterance.
// A status (too many frames, another configuration) stores nothing, so a stored row carries no error flag.  The layout of the
// header is part of the interface (include/e2e_ctc.h): 4-byte fields in this order, esum at byte 56.
constexpr unsigned kGramStreamMagic = 0x4d415247u;
constexpr int kGramStreamHeaderBytes = 256;
struct GramStreamHeader {
  unsigned magic;
  int V, K, R, W, scored, has_lm, restricted, max_frames;   // the configuration the row was written under (R: 0 unless scored)
  int n, frames, overflow, dead;         // members, frames consumed, the sticky overflow flag, 1: no hypothesis is left (n == 0)
  int pad;
  long long esum;                        // exponents taken out of the frames so far
};
static_assert(sizeof(GramStreamHeader) <= kGramStreamHeaderBytes && offsetof(GramStreamHeader, esum) == 56, "stream header");
constexpr int kGramStreamTooManyFrames = -2, kGramStreamOtherConfig = -3;
// what the streaming call adds to the whole call's parameters (whose x_len is then the chunk's lengths, T its width; ws holds
// no nodes).  cfg: the header a row of this call's configuration has, the run-time fields zero
struct GramStream {
  unsigned char* rows; size_t row_bytes, off_lm, off_nodes;   // (B,row_bytes); the LM fields and the node pool inside a row
  int64_t* frames_done;                  // (B): frames consumed so far, or the in-band status
  GramStreamHeader cfg;
};
// one block for the three ST instances: the plain one reads o.l.b alone
struct GramStreamParams { GramOptParams o; GramStream s; };
// one block for all the CUT instances: the stream's (a whole call reads its search's part) and the frames' lists, which
// launch_label_cut wrote on the same stream -- ids (B,T,S) with S = min(cutoff_top_n, V) + 1, cnt (B,T), T the call's
struct GramCutParams { GramStreamParams sp; const int32_t* ids; const int32_t* cnt; int S; };
template <bool LM, bool OPT, bool ST = false, bool CUT = false> using GramKernelParams = typename std::conditional<CUT, GramCutParams,
    typename std::conditional<ST, GramStreamParams,
    typename std::conditional<OPT, GramOptParams, typename std::conditional<LM, GramLmParams, GramBeamParams>::type>::type>::type>::type;
__device__ __forceinline__ const GramBeamParams& beam_of(const GramBeamParams& q) { return q; }
__device__ __forceinline__ const GramBeamParams& beam_of(const GramLmParams& q) { return q.b; }
__device__ __forceinline__ const GramBeamParams& search_of(const GramBeamParams& q) { return q; }
__device__ __forceinline__ const GramLmParams& search_of(const GramLmParams& q) { return q; }
__device__ __forceinline__ const GramLmParams& search_of(const GramOptParams& q) { return q.l; }
__device__ __forceinline__ int64_t* timesteps_of(const GramBeamParams&) { return nullptr; }
__device__ __forceinline__ int64_t* timesteps_of(const GramLmParams&) { return nullptr; }
__device__ __forceinline__ int64_t* timesteps_of(const GramOptParams& q) { return q.timesteps; }
__device__ __forceinline__ int64_t* timesteps_of(const GramStreamParams& q) { return q.o.timesteps; }
__device__ __forceinline__ GramStream stream_of(const GramBeamParams&) { return GramStream{}; }
__device__ __forceinline__ GramStream stream_of(const GramLmParams&) { return GramStream{}; }
__device__ __forceinline__ GramStream stream_of(const GramOptParams&) { return GramStream{}; }
__device__ __forceinline__ const GramStream& stream_of(const GramStreamParams& q) { return q.s; }
__device__ __forceinline__ int64_t* timesteps_of(const GramCutParams& q) { return q.sp.o.timesteps; }
__device__ __forceinline__ const GramStream& stream_of(const GramCutParams& q) { return q.sp.s; }
// the search's own block inside the kernel's: the stream's block holds the widest, of which an instance reads its part
template <bool LM, typename P> __device__ __forceinline__ const auto& search_in(const P& kp) {
  if constexpr (std::is_same<P, GramCutParams>::value) {
    if constexpr (LM) return kp.sp.o.l; else return kp.sp.o.l.b;
  } else if constexpr (std::is_same<P, GramStreamParams>::value) {
    if constexpr (LM) return kp.o.l; else return kp.o.l.b;
  } else return search_of(kp);
}
// the frames' lists of a CUT instance; the other blocks have none
template <typename P> __device__ __forceinline__ const int32_t* cut_ids_of(const P& kp) {
  if constexpr (std::is_same<P, GramCutParams>::value) return kp.ids; else return nullptr;
}
template <typename P> __device__ __forceinline__ const int32_t* cut_cnt_of(const P& kp) {
  if constexpr (std::is_same<P, GramCutParams>::value) return kp.cnt; else return nullptr;
}
template <typename P> __device__ __forceinline__ int cut_stride_of(const P& kp, int V) {
  if constexpr (std::is_same<P, GramCutParams>::value) return kp.S; else return V;
}

// the fields of one sequence, in registers
struct LmWalk {
  unsigned long long hash; double lm, lmb; int oov, oovb, nw, last, stn, stbn;
  unsigned st[kCtx], stb[kCtx];
};
__device__ __forceinline__ LmWalk load_walk(const LmMembers& L, int m) {
  LmWalk w;
  w.hash = L.hash[m]; w.lm = L.lm[m]; w.lmb = L.lmb[m]; w.oov = L.oov[m]; w.oovb = L.oovb[m];
  w.nw = L.nw[m]; w.last = L.last[m]; w.stn = L.stn[m]; w.stbn = L.stbn[m];
#pragma unroll
  for (int i = 0; i < kCtx; i++) { w.st[i] = L.st[i][m]; w.stb[i] = L.stb[i][m]; }
  return w;
}
__device__ __forceinline__ void store_walk(LmMembers& O, int r, const LmWalk& w) {
  O.hash[r] = w.hash; O.lm[r] = w.lm; O.lmb[r] = w.lmb; O.oov[r] = w.oov; O.oovb[r] = w.oovb;
  O.nw[r] = w.nw; O.last[r] = w.last; O.stn[r] = w.stn; O.stbn[r] = w.stbn;
#pragma unroll
  for (int i = 0; i < kCtx; i++) { O.st[i][r] = w.st[i]; O.stb[i][r] = w.stb[i]; }
}
__device__ __forceinline__ LmWalk root_walk(const GramLmParams& q) {
  LmWalk w;
  w.hash = kFnvInit; w.lm = 0.0; w.lmb = 0.0; w.oov = 0; w.oovb = 0; w.nw = 0; w.last = -1;
#pragma unroll
  for (int i = 0; i < kCtx; i++) { w.st[i] = 0u; w.stb[i] = 0u; }
  w.st[0] = q.has_lm ? q.lm.bos : 0u; w.stb[0] = w.st[0]; w.stn = 1; w.stbn = 1;
  return w;
}
// w: the fields of a sequence -> those of the sequence extended by column c's k base ids: get_next_prefix's LM part
// (asg_beam.hip's child_lm and what follows it there) applied id by id.  The model is asked where a word ends inside the
// gram and at the gram's last id; the answers in between would be overwritten (each is lm_before + one score, state_before
// + one word), so leaving them out changes no bit.  Without a model only the words are counted.
// LEX: the search restricted to the model's lexicon (e2e_gram_ctc_beam_nbest_opt).  The rule is applied id by id, but Pref(L)
// is prefix-closed, so the places where the model is asked anyway decide it: a word that ends inside the gram must be a word
// of L (an id, not the 0 of a mere prefix), the spelling at the gram's last id must be listed at all, and a gram that begins
// with the space needs the sequence's own last word to be one of L -- its last lookup counted no OOV.  -> false: the extended
// sequence is not admissible (there is no child; w is then of no use), found before the n-gram walk.  Without LEX: true.
template <bool LEX = false>
__device__ __forceinline__ bool walk_gram(const GramLmParams& q, LmWalk& w, int c, int k) {
  const int32_t* ids = q.b.gram_ids + c * kMaxK;
  int id = ids[0];
  for (int j = 0; j < k; j++) {
    const int nxt = j + 1 < k ? ids[j + 1] : -1;
    if constexpr (LEX) {                                          // a space after a word that the gram did not spell itself
      if (id == q.space_id && j == 0 && w.last >= 0 && w.last != q.space_id && w.oov != w.oovb) return false;
    }
    if (id != q.space_id) {                                       // (a space copies the fields)
      if (w.last < 0 || w.last == q.space_id) {                   // the id begins a word
        w.nw++;
        w.lmb = w.lm; w.oovb = w.oov; w.stbn = w.stn; w.hash = kFnvInit;
#pragma unroll
        for (int i = 0; i < kCtx; i++) w.stb[i] = w.st[i];
      }
      if (q.has_lm) {
        if ((unsigned)id < (unsigned)q.R) w.hash = spell(q.lm, w.hash, id);   // (the host cannot see the table: no id spells outside the strings)
        if (j + 1 == k || nxt == q.space_id) {
          uint32_t wi;
          if constexpr (LEX) {
            // (j + 1 < k: behind the gram's last id nxt is -1, which is also the space_id of a table without a space)
            if (!lm_word_find(q.lm, w.hash, wi) || (j + 1 < k && nxt == q.space_id && wi == 0)) return false;
          } else wi = lm_word_lookup(q.lm, w.hash);
          const float sc = lm_base_score(q.lm, w.stb, w.stbn, wi, nullptr, nullptr);
          w.lm = w.lmb + (double)sc / 2.302585092994045684;       // quirk Q8: divides by ln 10
          w.oov = w.oovb + (wi == 0 ? 1 : 0);
          int bn = w.stbn; if (bn > q.lm.order - 1) bn = q.lm.order - 1;
          int sn = bn + 1; if (sn > q.lm.order - 1) sn = q.lm.order - 1;
#pragma unroll
          for (int i = kCtx - 1; i >= 1; i--) w.st[i] = i < sn ? w.stb[i - 1] : 0u;
          w.st[0] = sn > 0 ? wi : 0u;
          w.stn = sn;
        }
      }
    }
    w.last = id;
    id = nxt;
  }
  return true;
}
// total = log tot + lmwt * lm_score - wip * num_words + oov_penalty * num_oov, in this order
__device__ __forceinline__ double total_of(const GramLmParams& q, double ac, double lm, int nw, int noov) {
  return ac + lm * q.lmwt - (double)nw * q.wip + (double)noov * q.oov;
}

// ---- the phases of a streaming call, compiled into the ST instances only ----
// What the row says before a chunk of Tc frames: the frames consumed so far (a fresh row: 0, resume = false) or a status < 0;
// n, esum, ovf: what the search resumes with.  The same for every thread of the workgroup (returned wave-uniform).
__device__ __forceinline__ int gram_stream_open(const GramStream& sp, const unsigned char* row, int Tc, bool& resume, int& n,
                                                long long& esum, int& ovf) {
  const GramStreamHeader h = *reinterpret_cast<const GramStreamHeader*>(row);
  const GramStreamHeader& c = sp.cfg;
  int st = 0, res = 0, nn = 1, ov = 0;
  long long es = 0;
  if (h.magic != 0u) {
    const bool same = h.magic == c.magic && h.V == c.V && h.K == c.K && h.R == c.R && h.W == c.W && h.scored == c.scored &&
                      h.has_lm == c.has_lm && h.restricted == c.restricted && h.max_frames == c.max_frames &&
                      h.n >= 0 && h.n <= c.W && h.dead == (h.n == 0 ? 1 : 0) && (h.overflow == 0 || h.overflow == 1) &&
                      h.frames >= 1 && h.frames <= c.max_frames;
    if (same) { st = h.frames; res = 1; nn = h.n; ov = h.overflow; es = h.esum; } else st = kGramStreamOtherConfig;
  }
  if (st >= 0 && st + Tc > c.max_frames) st = kGramStreamTooManyFrames;
  resume = __builtin_amdgcn_readfirstlane(res) != 0;
  n = __builtin_amdgcn_readfirstlane(nn);
  ovf = __builtin_amdgcn_readfirstlane(ov);
  esum = ((long long)__builtin_amdgcn_readfirstlane((int)(es >> 32)) << 32) |
         (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)es);
  return __builtin_amdgcn_readfirstlane(st);
}
static_assert(sizeof(Members) % 8 == 0 && sizeof(LmMembers) % 8 == 0, "the member sets are copied in 8-byte words");

// LM = false: the search on the masses alone (e2e_gram_ctc_beam_nbest), the parameter block GramBeamParams.  LM = true: the
// cut and the ranking on the totals with the language model's fields (e2e_gram_ctc_beam_nbest_lm).
// LEX (with LM): the search restricted to the model's lexicon -- the answer row of a member's children also says which of
// them there are (nw = kNoChild: none), and a pair without a child is dropped before it claims a table entry.  TS (with LM):
// the read-out also writes the frame each id's node was created at.  Instances of their own with a parameter block of their
// own: without LEX and TS the two kernels are the code they were, instruction for instruction (tools/diag/isa_compare.py).
// ST: the search fed in chunks (e2e_gram_ctc_beam_stream): resume from the state row, run the chunk's frames as frames f0 .. of
// the stream, suspend; the timesteps are then a run-time test on the pointer (TS is not read).  Without ST the code the kernel
// had before it could stream, instruction for instruction (profiles/gram_decode/isa_identity_stream.txt).
// CUT: the pruned search (e2e_gram_ctc_beam_nbest_cut, e2e_gram_ctc_beam_stream_cut; DESIGN.md 4.7, Pruned).  A frame expands the
// columns of its list alone -- a column outside it gives no extension share and no "run continues" share --, a pair's id is
// m * S + (the column's place in the list), and the table and the pair buffers hold W * S ids.  There is no answer cache: a
// pair's answer is walked from its parent's fields where it is needed (a function of the sequence alone: no bit changes), so
// a resumed stream has nothing to refill.  Without CUT the code the kernel had before, instruction for instruction
// (profiles/gram_cut/isa_identity.txt).
template <bool LM, bool LEX = false, bool TS = false, bool ST = false, bool CUT = false>
__global__ __launch_bounds__(kBeamThreads) void gram_beam_kernel(GramKernelParams<LM, LEX || TS, ST, CUT> kp) {
  static_assert(LM || !(LEX || TS), "the restricted search and the timesteps are the LM instance's");
  static_assert(!(ST && TS), "a stream tests the timesteps' pointer");
  const auto& q = search_in<LM>(kp);
  const GramBeamParams& p = beam_of(q);
  const GramStream& sp = stream_of(kp);
  __shared__ Members mem[2];
  __shared__ BeamCut cut;
  __shared__ int n_cand, n_surv, overflow;
  __shared__ unsigned long long sh_floor;
  __shared__ double sh_best;
  LmState* S = nullptr;
  Answer* cache = nullptr;                                       // [row][column], rows < 2 W
  if constexpr (LM) {
    __shared__ LmState lm_state;
    S = &lm_state;
    if constexpr (!CUT) cache = reinterpret_cast<Answer*>(p.ws + (size_t)blockIdx.x * p.per_utt + q.off_cache);
  }

  const int b = blockIdx.x, tid = threadIdx.x;
  const int V = p.V, K = p.K, W = p.W;
  const int PS = cut_stride_of(kp, V);                           // a pair's id is m * PS + c (CUT: + the place of c in the list)
  const int32_t* const cut_ids = cut_ids_of(kp);
  const int32_t* const cut_cnt = cut_cnt_of(kp);
  const unsigned n_ids = (unsigned)W * (unsigned)PS;
  unsigned char* ws = p.ws + (size_t)b * p.per_utt;
  double* y = reinterpret_cast<double*>(ws);
  Entry* table = reinterpret_cast<Entry*>(ws + p.off_table);
  int* next = reinterpret_cast<int*>(ws + p.off_next);
  int* list = reinterpret_cast<int*>(ws + p.off_list);
  double* ctot = reinterpret_cast<double*>(ws + p.off_tot);
  unsigned long long* sval = reinterpret_cast<unsigned long long*>(ws + p.off_sval);
  int* spos = reinterpret_cast<int*>(ws + p.off_spos);
  unsigned char* row = ST ? sp.rows + (size_t)b * sp.row_bytes : nullptr;   // the utterance's state row
  int2* nodes = reinterpret_cast<int2*>(ST ? row + sp.off_nodes : ws + p.off_nodes);
  const unsigned H = 1u << p.logH, hmask = H - 1u;
  const int64_t Tq = p.x_len[b];
  const int Tb = Tq < 0 ? 0 : (Tq > p.T ? p.T : (int)Tq);
  int f0 = 0, n0 = 1, ovf0 = 0;                                   // the stream's frames before this chunk; what it resumes with
  long long esum0 = 0;
  bool resume = false;
  if constexpr (ST) {
    f0 = gram_stream_open(sp, row, Tb, resume, n0, esum0, ovf0);
    // a status: nothing of the row or the utterance is touched
    if (f0 < 0) {
      if (tid == 0) { sp.frames_done[b] = f0; if (p.nbest) p.n_hyp[b] = f0; }
      return;
    }
  }

  for (unsigned i = tid; i < H; i += kBeamThreads) { table[i].key = 0ull; table[i].head = -1; }
  if constexpr (LM) { if (tid < kMaxW) { S->lms[0].row[tid] = 0; S->lms[1].row[tid] = 0; } }   // (never a row outside the cache)
  if (ST && resume) {                                            // the row's members become set 0
    stream_copy<kBeamThreads>(&mem[0], row + kGramStreamHeaderBytes, sizeof(Members));
    if constexpr (LM) stream_copy<kBeamThreads>(&S->lms[0], row + sp.off_lm, sizeof(LmMembers));
    if (tid == 0) overflow = ovf0;
  } else if (tid == 0) {
    for (int k = 0; k <= kMaxK; k++) { mem[0].p[k][0] = k == 0 ? 1.0 : 0.0; mem[0].col[k][0] = 0; }
    mem[0].key[0] = kKeyBasis; mem[0].tot[0] = 1.0; mem[0].node[0] = 0; mem[0].len[0] = 0;
    if (!ST || Tb > 0) nodes[0] = make_int2(-1, 0);              // (a chunk of no frames stores nothing)
    overflow = 0;
    if constexpr (LM) { store_walk(S->lms[0], 0, root_walk(q)); S->lms[0].row[0] = 0; }
  }
  __syncthreads();
  if constexpr (LM && !CUT) {
    if (ST && resume) {
      // the answer cache is not stored: the resumed members take rows 0 .. n - 1 and their children's answers are computed as
      // the per-frame refill computes a new member's.  They are functions of the sequence, so no bit depends on the row
      if (tid < kMaxW) S->lms[0].row[tid] = tid < n0 ? tid : 0;
      __syncthreads();
      if (q.has_lm && Tb > 0)
        for (int i = tid; i < n0 * V; i += kBeamThreads) {
          const int r = i / V, c = i - r * V;
          if (c == 0) continue;
          LmWalk w = load_walk(S->lms[0], r);
          const bool child = walk_gram<LEX>(q, w, c, order_of(p.gram_len, c, K));
          cache[(size_t)r * V + c] = Answer{w.lm, child ? w.nw : kNoChild, w.oov};
        }
    } else if (q.has_lm && Tb > 0)                                // the root's children, into row 0
      for (int c = 1 + tid; c < V; c += kBeamThreads) {
        LmWalk w = load_walk(S->lms[0], 0);
        const bool child = walk_gram<LEX>(q, w, c, order_of(p.gram_len, c, K));
        cache[c] = Answer{w.lm, child ? w.nw : kNoChild, w.oov};
      }
  }

  int cur = 0, n_mem = ST ? n0 : 1;
  long long esum = ST ? esum0 : 0;                              // exponents taken out of the frames so far
  for (int t = 0; t < Tb && n_mem > 0; t++) {
    const Members& M = mem[cur];
    Members& N = mem[cur ^ 1];
    // ---- the frame's probabilities ----
    const int32_t* kept = nullptr;                               // CUT: the frame's list and its length, 1 .. PS
    int n_kept = 0;
    if constexpr (CUT) {
      const int64_t frame = (int64_t)b * p.T + t;
      kept = cut_ids + frame * PS;
      const int n = cut_cnt[frame];
      n_kept = n < 1 ? 1 : (n > PS ? PS : n);
      const int64_t row = (int64_t)b * p.sB + (int64_t)t * p.sT;
      for (int j = tid; j < n_kept; j += kBeamThreads) {
        const int64_t at = row + (int64_t)kept_col(kept, j, V) * p.sV;
        const double v = p.dtype == E2E_F32 ? (double)reinterpret_cast<const float*>(p.lp)[at]
                                            : reinterpret_cast<const double*>(p.lp)[at];
        y[j] = exp(v);
      }
    } else {
      const int64_t row = (int64_t)b * p.sB + (int64_t)t * p.sT;
      for (int c = tid; c < V; c += kBeamThreads) {
        const int64_t at = row + (int64_t)c * p.sV;
        const double v = p.dtype == E2E_F32 ? (double)reinterpret_cast<const float*>(p.lp)[at]
                                            : reinterpret_cast<const double*>(p.lp)[at];
        y[c] = exp(v);
      }
    }
    if (tid == 0) { n_cand = 0; n_surv = 0; cut.n_sel = 0; sh_floor = ~0ull; }
    if constexpr (LM) {
      if (tid < 2 * kMaxW) S->used[tid] = 0;
      if (tid == 0) { S->n_stay = 0; S->n_new = 0; S->n_free = 0; }
    }
    __syncthreads();
    // ---- members and (member, column) pairs meet at their prefix's key ----
    const unsigned n_now = (unsigned)n_mem * (unsigned)(CUT ? n_kept : V);
    for (unsigned it = tid; it < n_now; it += kBeamThreads) {
      unsigned id = it, m, c, at;                                // at: the column's place in y
      if constexpr (CUT) {
        m = it / (unsigned)n_kept; at = it - m * (unsigned)n_kept;
        id = m * (unsigned)PS + at;
        c = (unsigned)kept_col(kept, (int)at, V);
        if (at != 0 && c == 0) continue;                         // (no column of the table: see kept_col)
      } else {
        m = id / (unsigned)V; c = id - m * (unsigned)V; at = c;
      }
      unsigned long long key = M.key[m];
      bool go = true;
      if (c != 0) {
        const int k = order_of(p.gram_len, (int)c, K);
        go = ext_source(M, (int)m, k, (int)c, K) * y[at] > 0.0;
        if constexpr (LEX) {
          if constexpr (CUT) {                                   // (no child: no candidate -- asked of the parent's fields on the spot)
            if (go) { LmWalk w = load_walk(S->lms[cur], (int)m); go = walk_gram<true>(q, w, (int)c, k); }
          } else go = go && cache[(size_t)S->lms[cur].row[m] * V + c].nw != kNoChild;   // (no child: no candidate)
        }
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
      eval_cand<CUT>(E, M, head, next, y, kept, n_kept, p.gram_len, (unsigned)PS, V, K, n_ids);
      const double tot = eval_total(E, K);
      if constexpr (LM) {
        // the order key of the total; the fields are the member's own where the prefix stays, else its smallest pair's
        // (a model's answers from the parent's row, the words alone counted on the spot)
        const LmMembers& L = S->lms[cur];
        unsigned long long cand = kNoCand;
        if (tot > 0.0) {
          Answer a;
          if (E.stay >= 0) a = Answer{L.lm[E.stay], L.nw[E.stay], L.oov[E.stay]};
          else {
            const unsigned pid = (unsigned)E.pair < n_ids ? (unsigned)E.pair : 0u;
            const unsigned pm = pid / (unsigned)PS;
            const unsigned pc = CUT ? (unsigned)kept_col(kept, (int)(pid - pm * (unsigned)PS), V) : pid - pm * (unsigned)PS;
            if constexpr (CUT) {                                  // (no cache: the parent's fields walked through the gram)
              LmWalk w = load_walk(L, (int)pm);
              (void)walk_gram<LEX>(q, w, (int)pc, order_of(p.gram_len, (int)pc, K));
              a = Answer{w.lm, w.nw, w.oov};
            } else if (q.has_lm) a = cache[(size_t)L.row[pm] * V + pc];
            else {
              LmWalk w = load_walk(L, (int)pm);
              walk_gram(q, w, (int)pc, order_of(p.gram_len, (int)pc, K));
              a = Answer{0.0, w.nw, 0};
            }
          }
          const double total = total_of(q, log(tot), a.lm, a.nw, a.oov);
          if (total > ninf()) {                                   // (false for NaN as well)
            cand = okey(total);
            if (E.stay >= 0) { atomicMin(&sh_floor, cand); atomicAdd(&S->n_stay, 1); }
          }
        }
        reinterpret_cast<unsigned long long*>(ctot)[pos] = cand;
      } else {
        ctot[pos] = tot;
        if (E.stay >= 0) atomicMin(&sh_floor, tot > 0.0 ? (unsigned long long)__double_as_longlong(tot) : 0ull);
      }
    }
    __syncthreads();
    // ---- an exact filter: a full beam's members are W candidates themselves, so nothing below the least of them can
    //      make the cut; what is left (usually a few times W) is what the selection reads ----
    if constexpr (LM) {                                          // (on the totals' order keys: the members that ARE candidates)
      const unsigned long long floor_bits = S->n_stay == W ? sh_floor : 1ull;
      for (int pos = tid; pos < nc; pos += kBeamThreads) {
        const unsigned long long v = reinterpret_cast<const unsigned long long*>(ctot)[pos];
        if (v < floor_bits) continue;                            // (kNoCand = 0 is below both)
        const int j = atomicAdd(&n_surv, 1);
        sval[j] = v; spos[j] = pos;
      }
    } else {
      const unsigned long long floor_bits = n_mem == W ? sh_floor : 0ull;
      for (int pos = tid; pos < nc; pos += kBeamThreads) {
        const double tot = ctot[pos];
        const unsigned long long v = (unsigned long long)__double_as_longlong(tot);
        if (!(tot > 0.0) || v < floor_bits) continue;            // (NaN totals, from NaN inputs, are no members either)
        const int j = atomicAdd(&n_surv, 1);
        sval[j] = v; spos[j] = pos;
      }
    }
    __syncthreads();
    // ---- the cut: the W largest totals, exactly equal ones by ascending key ----
    const auto key_at = [&](int pos) { return __hip_atomic_load(&table[list[pos]].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    if constexpr (LM) beam_cut<kBeamThreads>(cut, sval, spos, n_surv, W, key_at, okey_inv);
    else beam_cut<kBeamThreads>(cut, sval, spos, n_surv, W, key_at,
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
    if constexpr (LM) {                                          // (sel_tot is the total: the rescale wants the best's mass)
      if (tid < ns && cut.sel_rank[tid] == 0) {
        const int head = __hip_atomic_load(&table[list[cut.sel_pos[tid]]].head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        Eval E;
        eval_cand<CUT>(E, M, head, next, y, kept, n_kept, p.gram_len, (unsigned)PS, V, K, n_ids);
        sh_best = eval_total(E, K);
      }
    } else {
      if (tid < ns && cut.sel_rank[tid] == 0) sh_best = cut.sel_tot[tid];
    }
    __syncthreads();
    int ex = 0;
    (void)frexp(sh_best, &ex);                                   // best = f * 2^ex, f in [0.5, 1)
    if (tid < ns) {
      const int pos = cut.sel_pos[tid], r = cut.sel_rank[tid];
      const int head = __hip_atomic_load(&table[list[pos]].head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      Eval E;
      eval_cand<CUT>(E, M, head, next, y, kept, n_kept, p.gram_len, (unsigned)PS, V, K, n_ids);
      double tot = 0.0;
#pragma unroll
      for (int k = 0; k <= kMaxK; k++) {
        const double pk = k <= K ? ldexp(E.s[k], -ex) : 0.0;
        N.p[k][r] = pk; N.col[k][r] = (k >= 1 && pk > 0.0) ? E.c[k] : 0;
        if (k <= K) tot += pk;
      }
      N.tot[r] = tot; N.key[r] = cut.sel_key[tid];
      if (E.stay >= 0) {
        N.node[r] = M.node[E.stay]; N.len[r] = M.len[E.stay];
        if constexpr (LM) {                                      // the fields and the row of answers stay the member's
          const LmMembers& L = S->lms[cur];
          store_walk(S->lms[cur ^ 1], r, load_walk(L, E.stay));
          if constexpr (!CUT) {
            S->lms[cur ^ 1].row[r] = L.row[E.stay];
            S->used[L.row[E.stay]] = 1;
          }
        }
      } else {
        const unsigned pid = (unsigned)E.pair < n_ids ? (unsigned)E.pair : 0u;
        const unsigned pm = pid / (unsigned)PS;
        const unsigned pc = CUT ? (unsigned)kept_col(kept, (int)(pid - pm * (unsigned)PS), V) : pid - pm * (unsigned)PS;
        const int node = 1 + (ST ? f0 + t : t) * W + r;          // (a stream's nodes count the stream's frames)
        nodes[node] = make_int2(M.node[pm], (int)pc);
        N.node[r] = node; N.len[r] = M.len[pm] + order_of(p.gram_len, (int)pc, K);
        if constexpr (LM) {                                      // a new prefix: its parent's fields walked through the gram
          LmWalk w = load_walk(S->lms[cur], (int)pm);
          (void)walk_gram<LEX>(q, w, (int)pc, order_of(p.gram_len, (int)pc, K));   // (a pair that was not dropped: a child)
          store_walk(S->lms[cur ^ 1], r, w);
          if constexpr (!CUT) S->new_list[atomicAdd(&S->n_new, 1)] = (unsigned char)r;
        }
      }
    }
    __syncthreads();                                             // (the lists above are read to the end before they go)
    // ---- free the frame's entries ----
    for (int pos = tid; pos < nc; pos += kBeamThreads) { Entry& en = table[list[pos]]; en.key = 0ull; en.head = -1; }
    if constexpr (LM && !CUT) {
      // ---- the new members take the rows that no staying member holds (at least W of the 2 W), and the answers of their
      //      children are computed once: lm_score, num_words, num_oov of (member, column), read by the cuts to come ----
      LmMembers& O = S->lms[cur ^ 1];
      if (q.has_lm) {
        if (tid < 2 * W && !S->used[tid]) S->free_list[atomicAdd(&S->n_free, 1)] = (unsigned char)tid;
        __syncthreads();
        const int n_new = S->n_new;
        if (tid < n_new) O.row[S->new_list[tid]] = S->free_list[tid];
        __syncthreads();
        for (int i = tid; i < n_new * V; i += kBeamThreads) {
          const int j = i / V, c = i - j * V;
          if (c == 0) continue;
          const int r = S->new_list[j];
          LmWalk w = load_walk(O, r);
          const bool child = walk_gram<LEX>(q, w, c, order_of(p.gram_len, c, K));
          cache[(size_t)O.row[r] * V + c] = Answer{w.lm, child ? w.nw : kNoChild, w.oov};
        }
      }
    }
    esum += ex; n_mem = ns; cur ^= 1;
    __syncthreads();
  }

  // ---- suspend, behind the chunk's last frame: the current set, then the header.  A chunk of no frames stores nothing ----
  if constexpr (ST) {
    if (Tb > 0) {
      stream_copy<kBeamThreads>(row + kGramStreamHeaderBytes, &mem[cur], sizeof(Members));
      if constexpr (LM) stream_copy<kBeamThreads>(row + sp.off_lm, &S->lms[cur], sizeof(LmMembers));
    }
    if (tid == 0) {
      if (Tb > 0) {
        GramStreamHeader h = sp.cfg;
        h.n = n_mem; h.frames = f0 + Tb; h.overflow = overflow ? 1 : 0; h.dead = n_mem == 0 ? 1 : 0; h.pad = 0; h.esum = esum;
        *reinterpret_cast<GramStreamHeader*>(row) = h;
      }
      sp.frames_done[b] = f0 + Tb;
    }
    if (p.nbest == 0) return;                                    // feed only
  }

  // ---- read-out: the first nbest members, ranked already ----
  const Members& F = mem[cur];
  const int nbest = p.nbest;
  const int64_t max_out = p.max_out;
  const bool want_ts = ST ? timesteps_of(kp) != nullptr : TS;
  const int max_hops = ST ? f0 + Tb : p.T;                       // a sequence has at most one node per frame consumed
  int64_t* out = p.out + (int64_t)b * nbest * max_out;
  int64_t* ts = nullptr;
  if (want_ts) ts = timesteps_of(kp) + (int64_t)b * nbest * max_out;
  if (tid < nbest) {
    int64_t* row = out + (int64_t)tid * max_out;
    int64_t* trow = nullptr;
    if (want_ts) trow = ts + (int64_t)tid * max_out;
    int len = 0; double score = -__builtin_huge_val();
    if (tid < n_mem) {
      len = F.len[tid];
      score = log(F.tot[tid]) + (double)esum * 0.6931471805599453094;
      int at = len, node = F.node[tid];
      for (int hops = 0; node > 0 && hops <= max_hops; hops++) {
        if constexpr (ST) { if (node > W * sp.cfg.max_frames) break; }   // (no node of this row's pool: the row is not this call's)
        const int2 nd = nodes[node];
        const int k = order_of(p.gram_len, nd.y, K);
        for (int j = k - 1; j >= 0; j--) {
          --at;
          if (at >= 0 && at < max_out) {
            row[at] = (int64_t)p.gram_ids[nd.y * kMaxK + j];
            if (want_ts) trow[at] = (int64_t)((node - 1) / W);   // node = 1 + t * W + rank: a gram's ids share the frame
          }
        }
        node = nd.x;
      }
    }
    cut.sel_pos[tid] = len;
    p.out_len[(int64_t)b * nbest + tid] = len;
    if constexpr (LM) {                                          // scores: total, ac, lm_score; counts: words, OOVs
      const int64_t o = (int64_t)b * nbest + tid;
      double lm = 0.0, tot = score; int nw = 0, noov = 0;
      if (tid < n_mem) {
        const LmMembers& L = S->lms[cur];
        lm = L.lm[tid]; nw = L.nw[tid]; noov = L.oov[tid];
        tot = total_of(q, score, lm, nw, noov);
      }
      p.scores[o * 3 + 0] = tot; p.scores[o * 3 + 1] = score; p.scores[o * 3 + 2] = lm;
      q.counts[o * 2 + 0] = nw; q.counts[o * 2 + 1] = noov;
    } else {
      p.scores[(int64_t)b * nbest + tid] = score;
    }
  }
  __syncthreads();
  for (int j = 0; j < nbest; j++) {
    int64_t* row = out + (int64_t)j * max_out;
    for (int64_t i = cut.sel_pos[j] + tid; i < max_out; i += kBeamThreads) row[i] = 0;
    if (want_ts) for (int64_t i = cut.sel_pos[j] + tid; i < max_out; i += kBeamThreads) ts[(int64_t)j * max_out + i] = -1;
  }
  if (tid == 0) p.n_hyp[b] = overflow ? -1 : (n_mem < nbest ? n_mem : nbest);
}

struct BeamLayout { size_t per_utt, off_table, off_next, off_list, off_tot, off_sval, off_spos, off_nodes, off_cache; int logH; };

// with_lm: behind the nodes the children's answers of 2 W prefixes, 16 bytes per (row, column)
bool beam_layout(int T, int V, int K, int W, BeamLayout& L, bool with_lm = false) {
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
  L.off_cache = at; if (with_lm) at += align_up(2 * ids * sizeof(Answer), 256);
  L.per_utt = at; L.logH = logH;
  return true;
}

// every argument error of the two n-best calls that the host can see, before any launch
// (cut_top_n > 0: a pruned call, whose width limit is e2e_gram_beam_cut_max_width's)
int check_beam_args(int dtype, int B, int T, int V, int max_order, int beam_width, int nbest, int64_t max_out, int min_nbest = 1,
                    int cut_top_n = 0) {
  if (dtype != E2E_F32 && dtype != E2E_F64) { set_error("dtype must be E2E_F32 or E2E_F64"); return E2E_ERR_ARG; }
  if (B < 0 || T < 1 || V < 1 || max_out < 0) { set_error("bad sizes B=%d T=%d V=%d max_out=%lld", B, T, V, (long long)max_out); return E2E_ERR_ARG; }
  if (max_order < 1 || max_order > kMaxK) { set_error("max_order %d is not in [1, %d]", max_order, kMaxK); return E2E_ERR_ARG; }
  if (beam_width < 1) { set_error("beam_width %d must be at least 1", beam_width); return E2E_ERR_ARG; }
  if (cut_top_n > 0) {
    if (beam_width > e2e_gram_beam_cut_max_width(V, max_order, cut_top_n)) {
      set_error("beam_width %d exceeds e2e_gram_beam_cut_max_width(V=%d, max_order=%d, cutoff_top_n=%d) = %d", beam_width, V, max_order,
                cut_top_n, e2e_gram_beam_cut_max_width(V, max_order, cut_top_n));
      return E2E_ERR_UNSUPPORTED;
    }
  } else if (beam_width > e2e_gram_beam_max_width(V, max_order)) {
    set_error("beam_width %d exceeds e2e_gram_beam_max_width(V=%d, max_order=%d) = %d", beam_width, V, max_order,
              e2e_gram_beam_max_width(V, max_order));
    return E2E_ERR_UNSUPPORTED;
  }
  if (nbest < min_nbest || nbest > beam_width) { set_error("nbest=%d outside [%d, beam_width=%d]", nbest, min_nbest, beam_width); return E2E_ERR_ARG; }
  return E2E_OK;
}

// ... of the scored calls (e2e_gram_ctc_beam_nbest_opt and the scored stream): the base labels, the space, the model
int check_scored_args(int V, int num_base_labels, int space_id, const e2e_lm* lm, bool restricted) {
  if (num_base_labels < 1 || num_base_labels > V) { set_error("num_base_labels=%d outside [1, V=%d]", num_base_labels, V); return E2E_ERR_ARG; }
  if (space_id >= num_base_labels) { set_error("space_id=%d is not one of the %d base labels", space_id, num_base_labels); return E2E_ERR_ARG; }
  if (lm) {
    if (lm->transcribed || (lm->words_only && !restricted)) {
      set_error("the Gram-CTC search spells its words from the base labels' strings: a model with custom transcriptions "
                "(e2e_lm_load_transcriptions) is not supported, and a word list (e2e_lm_load_words) only by a search that is "
                "restricted to it (e2e_gram_ctc_beam_nbest_opt, restrict_to_lexicon)");
      return E2E_ERR_ARG;
    }
    if (lm->order > kLmMaxOrder) { set_error("a language model of order %d: at most %d", lm->order, kLmMaxOrder); return E2E_ERR_ARG; }
    if ((int)lm->label_off.size() - 1 != num_base_labels) {
      set_error("the language model was loaded with %d labels but the table has num_base_labels=%d",
                (int)lm->label_off.size() - 1, num_base_labels);
      return E2E_ERR_ARG;
    }
  }
  return check_lexicon(lm, restricted);
}
// (... and the device the model's tables are on: check_model_device, ctc_lm.h)

// ... the null-pointer test of a call on B > 0 utterances: the pointers it needs, in any order.  (A pointer that this call does
// not need -- out without room for an id, counts of an unscored search -- is given as `unused`)
const void* const unused = &unused;
int check_pointers(int B, std::initializer_list<const void*> needed) {
  for (const void* p : needed) if (B > 0 && !p) { set_error("null pointer argument"); return E2E_ERR_ARG; }
  return E2E_OK;
}
// ... and the workspace: aligned, then at least `need` bytes -- what the entry's query, named `query`, says, less its slack
int check_workspace(void*& workspace, size_t& workspace_bytes, size_t need, const char* query) {
  if (align_workspace(workspace, workspace_bytes) && workspace_bytes >= need) return E2E_OK;
  set_error("workspace too small: %zu bytes, %s() = %zu", workspace_bytes, query, need + 256);
  return E2E_ERR_WORKSPACE;
}

// the search's parameter block, the whole call's and the stream's alike; where the nodes lie (per_utt, off_nodes) is the caller's
void fill_params(GramBeamParams& p, const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len, int B, int T,
                 int V, const int32_t* gram_ids, const int32_t* gram_len, int max_order, int beam_width, int nbest, int64_t* out,
                 int64_t max_out, int64_t* out_len, int64_t* n_hyp, double* scores, void* workspace, const BeamLayout& L,
                 size_t per_utt, size_t off_nodes) {
  p = GramBeamParams{lp, dtype, sB, sT, sV, x_len, B, T, V, gram_ids, gram_len, max_order, beam_width, nbest,
                     out, max_out, out_len, n_hyp, scores, reinterpret_cast<unsigned char*>(workspace),
                     per_utt, L.off_table, L.off_next, L.off_list, L.off_tot, L.off_sval, L.off_spos, off_nodes, L.logH};
}
// ... and what a scored search adds to it
void fill_lm_params(GramLmParams& q, int num_base_labels, int space_id, const e2e_lm* lm, double lmwt, double wip, double oov_penalty,
                    int32_t* counts, const BeamLayout& L) {
  if (lm) q.lm = lm->dev_view(); else memset(&q.lm, 0, sizeof(q.lm));
  q.has_lm = lm ? 1 : 0; q.space_id = space_id < 0 ? -1 : space_id; q.R = num_base_labels;
  q.lmwt = lm ? lmwt : 0.0; q.wip = wip; q.oov = oov_penalty;
  q.counts = counts; q.off_cache = L.off_cache;
}

// a state row of a stream: header | Members | LmMembers (scored) | node pool of max_frames frames, each part 256-aligned.  The
// workspace of a streaming call: a frame's scratch (beam_layout's up to the nodes, which are the row's) and, with a model,
// the answer cache in the nodes' place
struct StreamLayout { size_t off_lm, off_nodes, total, ws_per_utt; };
bool stream_layout(int max_frames, int V, int K, int W, bool scored, bool with_lm, StreamLayout& S, BeamLayout& L) {
  if (max_frames < 1 || max_frames > (1 << 22) || (with_lm && !scored) || !beam_layout(1, V, K, W, L, with_lm)) return false;
  S.off_lm = kGramStreamHeaderBytes + align_up(sizeof(Members), 256);
  S.off_nodes = S.off_lm + (scored ? align_up(sizeof(LmMembers), 256) : 0);
  S.total = S.off_nodes + align_up(((size_t)W * ((size_t)max_frames + 1) + 1) * 8, 256);
  S.ws_per_utt = L.off_nodes + (L.per_utt - L.off_cache);
  L.off_cache = L.off_nodes;
  return true;
}

}  // namespace
}  // namespace e2e
