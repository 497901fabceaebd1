// ASG prefix beam search with transitions and a word language model (the definition: include/e2e_ctc.h, beside the ASG loss):
// asg_beam_kernel and the host code of its calls.
//
// One workgroup per utterance, serial in t.  The beam's members (up to 128 label sequences: log mass, last label, 64-bit key,
// read-out node and, with a model, the LM fields of ctc_beam.hip's prefixes) live in LDS, double buffered.
//
// What makes this search simpler than the Gram-CTC one (ctc_gram_decode.hip) is that a sequence has ONE parent: the candidate
// y + (c) is reached by the pair (member y, label c) and by nothing else, so two pairs never meet.  A pair can only meet a
// MEMBER -- the one that is y + (c) already and also stays.  So there is no table of candidates in memory: the members' keys sit in
// a 512-slot open-addressing table in LDS, every pair looks its key up there, and a pair that finds a member leaves its share
// in that member's `ext` cell (one writer: the parent is unique).  A candidate's mass is then log-sum(stay, ext) -- two terms,
// symmetric in its arguments -- or the pair's share alone; no atomics on numbers, the same bits on every call.
// The per-frame cut first drops what cannot matter (a full beam's members are W candidates themselves: nothing below the
// least of their new totals survives); the select and the ranking are beam_cut.h's, the select on the order-preserving
// bits of the totals, and the survivors become the next members in the order of their ranks.
// The read-out walks the (parent node, label) pool backwards; a node's index, 1 + t * W + rank, also says at which frame its
// sequence was created (the optional timesteps).
// Restricted to the model's lexicon (e2e_asg_beam_nbest_opt, the LEX instances): a pair whose sequence is not admissible is
// no candidate -- one probe of the vocabulary table for a label, the member's own OOV counts for the space.
//
// The search can stop after any frame and go on in a later launch (e2e_asg_beam_stream, the ST instances): what a frame hands
// to the next is one member set (with a model: its LM fields too), the member count and the node pool.  They live in a state
// row of the caller's (AsgStreamHeader | Members | LmMembers | nodes); the key table is rebuilt from the members' keys at
// resume, ctot / sval / spos are a frame's scratch.  A node's index counts the frames of the STREAM, so the timesteps need nothing.
//
// The transitions are read from an f64 copy in the workspace, transposed to [from][to] by a small kernel of the same call: the
// pairs of one member read one contiguous row (see DESIGN.md 4.10 for why not LDS).
//
// This header is the kernel and the host code both objects share: asg_beam.hip (the unpruned instances and entries) and
// asg_beam_cut.hip (the pruned ones, CUT).
#pragma once
#include <cstring>
#include <type_traits>

#include "beam_cut.h"
#include "ctc_lm.h"

namespace e2e {
namespace {

constexpr int kThreads = 1024;
constexpr int kMaxV = 128;                 // e2e_asg_max_labels()
constexpr int kMaxPairs = 16384;           // beam_width * V
constexpr int kSlots = 512;                // the members' key table (<= 25 % full)
constexpr unsigned long long kNoCand = 0ull;   // okey() of nothing: below every number's key (okey(-inf) = 0x000f...f)

// (okey: beam_cut.h) ... and back
__device__ __forceinline__ double okey_inv(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}
// log(exp(a) + exp(b)), symmetric in a and b (so no result depends on which share is called which); -inf is "no share"
__device__ __forceinline__ double lse_sym(double a, double b) {
  const double hi = a > b ? a : b, lo = a > b ? b : a;
  if (lo == ninf()) return hi;
  return hi + log1p(exp(lo - hi));
}
__device__ __forceinline__ unsigned long long child_key(unsigned long long key, int c) {
  const unsigned long long k = (key ^ (unsigned long long)(unsigned)c) * kKeyPrime;
  return k == 0ull ? 1ull : k;
}

struct Members {
  double s[kMaxW];                       // log mass
  unsigned long long key[kMaxW];
  int last[kMaxW];                       // last label; -1: the root (frame 0 only)
  int node[kMaxW], len[kMaxW], nw[kMaxW];
};
// the LM fields of a member (ctc_beam.hip's LmFields, as arrays)
struct LmMembers {
  unsigned long long hash[kMaxW];        // running FNV hash of the last word's expanded spelling
  double lm[kMaxW], lmb[kMaxW];          // lm_score, lm_before
  int oov[kMaxW], oovb[kMaxW];
  unsigned st[kCtx][kMaxW], stb[kCtx][kMaxW];   // LM context after / before the last word, most recent first
  int stn[kMaxW], stbn[kMaxW];
};
struct NoLm {};

struct AsgBeamParams {
  const void* x; int dtype; int64_t sB, sT, sV; const int64_t* x_len;
  int B, T, V, R, W, space_id, nbest;
  LmView lm; double lmwt, wip, oov;
  int64_t* out; int64_t max_out; int64_t* out_len; int64_t* n_hyp; double* scores; int32_t* counts;
  const double* At;                      // [from][to], f64
  unsigned char* ws; size_t per_utt, off_sval, off_spos, off_nodes;
  int64_t* timesteps;                    // (B,nbest,max_out): the frame each label's node was created at; the TS instances only
};

// ---- the state row of a stream (e2e_asg_beam_stream): header (256 bytes) | Members | LmMembers (with a model) | node pool ----
// Indices only, never an address: a row may be moved or copied.  magic == 0 -- what a zeroed header has -- is a fresh utterance.
// A status (too many frames, another configuration) stores nothing, so a stored row carries no error flag.
constexpr unsigned kAsgStreamMagic = 0x53475341u;
constexpr int kAsgStreamHeaderBytes = 256;
struct AsgStreamHeader {
  unsigned magic;
  int V, R, W, has_lm, max_frames;       // the configuration the row was written under
  int n, frames, dead;                   // members, frames consumed, 1: no hypothesis is left (then n == 0)
};
static_assert(sizeof(AsgStreamHeader) <= kAsgStreamHeaderBytes, "stream header");
constexpr int kAsgStreamTooManyFrames = -2, kAsgStreamOtherConfig = -3;
// what the streaming call adds to AsgBeamParams (whose x_len is then the chunk's lengths, T its width; ws holds no nodes)
struct AsgStream {
  unsigned char* rows; size_t row_bytes, off_lm, off_nodes;   // (B,row_bytes); the LM fields and the node pool inside a row
  int max_frames;
  int64_t* frames_done;                  // (B): frames consumed so far, or the in-band status
};
struct AsgStreamParams { AsgBeamParams b; AsgStream s; };
// ---- the pruned search (CUT, asg_beam_cut.hip): one block for all its instances, the stream's (a whole call reads its
// search's part) and the frames' lists: ids (B,T,K) int32, a frame's K kept labels in ascending id; K = min(cutoff_top_n, V)
struct AsgCutParams { AsgStreamParams sp; const int32_t* ids; int K; };
// the kernel's parameter block: the ST instances take the stream's, the CUT instances theirs, the others the one they always took
template <bool ST, bool CUT = false> using AsgKernelParams =
    typename std::conditional<CUT, AsgCutParams, typename std::conditional<ST, AsgStreamParams, AsgBeamParams>::type>::type;
__device__ __forceinline__ const AsgBeamParams& beam_of(const AsgBeamParams& q) { return q; }
__device__ __forceinline__ const AsgBeamParams& beam_of(const AsgStreamParams& q) { return q.b; }
__device__ __forceinline__ const AsgBeamParams& beam_of(const AsgCutParams& q) { return q.sp.b; }
__device__ __forceinline__ AsgStream stream_of(const AsgBeamParams&) { return AsgStream{}; }
__device__ __forceinline__ const AsgStream& stream_of(const AsgStreamParams& q) { return q.s; }
__device__ __forceinline__ const AsgStream& stream_of(const AsgCutParams& q) { return q.sp.s; }
// the frames' lists and the pairs of a member (a frame's kept labels; without CUT every label)
template <typename P> __device__ __forceinline__ const int32_t* cut_ids_of(const P& q) {
  if constexpr (std::is_same<P, AsgCutParams>::value) return q.ids; else return nullptr;
}
template <typename P> __device__ __forceinline__ int cut_pairs_of(const P& q, int V) {
  if constexpr (std::is_same<P, AsgCutParams>::value) return q.K; else return V;
}
// the LDS of a CUT frame: its list, and where a label stands in it (-1: not kept)
struct CutFrame { int kept[kMaxV]; int place_of[kMaxV]; };
// the label of a member's pair j: j itself, or (CUT) the list's entry j
template <bool CUT, typename F> __device__ __forceinline__ int label_at(const F& cf, int j) {
  if constexpr (CUT) return cf.kept[j]; else return j;
}

// may label c follow a sequence that ends in `a` (a == -1: nothing yet)?  c != a is the caller's.
__device__ __forceinline__ bool spellable(const AsgBeamParams& p, int a, int c) {
  const int nch = p.V - p.R;
  return c < nch || (a >= 0 && a < nch && a != p.space_id);
}

// what the pair (member m, label c != space) asks of the model: the expanded word's hash, its id, its score in the context
// (`listed`, the restricted search's: the spelling is in the table at all -- a word, or with id 0 a prefix of one)
struct LmAnswer { unsigned long long h; uint32_t wi; float sc; bool listed; };
template <bool LEX = false>
__device__ __forceinline__ LmAnswer lm_query(const AsgBeamParams& p, const LmMembers& L, int m, int a, int c, bool new_word) {
  LmAnswer ans;
  unsigned long long h = new_word ? kFnvInit : L.hash[m];
  const int nch = p.V - p.R;
  if (c >= nch) { for (int r = c - nch; r >= 0; r--) h = spell(p.lm, h, a); }     // repeat label: `a` again, c - nch + 1 times
  else h = spell(p.lm, h, c);
  uint32_t ctx[kCtx];
  const int cn = new_word ? L.stn[m] : L.stbn[m];
#pragma unroll
  for (int i = 0; i < kCtx; i++) ctx[i] = new_word ? L.st[i][m] : L.stb[i][m];
  ans.h = h;
  if constexpr (LEX) ans.listed = lm_word_find(p.lm, h, ans.wi);
  else { ans.wi = lm_word_lookup(p.lm, h); ans.listed = true; }
  if (LEX && !ans.listed) { ans.sc = 0.f; return ans; }           // no candidate: nothing to score
  ans.sc = lm_base_score(p.lm, ctx, cn, ans.wi, nullptr, nullptr);
  return ans;
}

// total = ac + lmwt * lm_score - wip * num_words + oov_penalty * num_oov, in this order
__device__ __forceinline__ double total_of(const AsgBeamParams& p, double ac, double lm, int nw, int noov) {
  return ac + lm * p.lmwt - (double)nw * p.wip + (double)noov * p.oov;
}
// the mass of member m's sequence (last label a) extended by label c != a: the share of the pair (m, c)
__device__ __forceinline__ double ext_mass(const AsgBeamParams& p, const Members& M, const double* xs, int m, int a, int c) {
  return a < 0 ? xs[c] : M.s[m] + p.At[a * p.V + c] + xs[c];
}
// the mass of member m (last label a >= 0) once it has stayed on a and taken its extension share
__device__ __forceinline__ double stay_mass(const AsgBeamParams& p, const Members& M, const double* xs, const double* ext, int m, int a) {
  return lse_sym(M.s[m] + p.At[a * p.V + a] + xs[a], ext[m]);
}
// does label c, after a sequence that ends in `a`, begin a word?
__device__ __forceinline__ bool new_word(const AsgBeamParams& p, int a, int c) {
  return c != p.space_id && (a < 0 || a == p.space_id);
}
// O[r] = L[m]
__device__ __forceinline__ void copy_lm(LmMembers& O, int r, const LmMembers& L, int m) {
  O.hash[r] = L.hash[m]; O.lm[r] = L.lm[m]; O.lmb[r] = L.lmb[m]; O.oov[r] = L.oov[m]; O.oovb[r] = L.oovb[m];
#pragma unroll
  for (int i = 0; i < kCtx; i++) { O.st[i][r] = L.st[i][m]; O.stb[i][r] = L.stb[i][m]; }
  O.stn[r] = L.stn[m]; O.stbn[r] = L.stbn[m];
}
// the LM score and the OOV count of member m's child by a label that is no space: before its last word (m's own where the
// child begins a word) and with it
struct ChildLm { double lmb, lm; int oovb, oov; };
__device__ __forceinline__ ChildLm child_lm(const LmMembers& L, int m, bool nw, const LmAnswer& ans) {
  ChildLm s;
  s.lmb = nw ? L.lm[m] : L.lmb[m];
  s.oovb = nw ? L.oov[m] : L.oovb[m];
  s.lm = s.lmb + (double)ans.sc / 2.302585092994045684;         // quirk Q8: divides by ln 10
  s.oov = s.oovb + (ans.wi == 0 ? 1 : 0);
  return s;
}

// the key of new member r enters the table (two members with one key, 2^-64: the second is not entered and never extended into)
__device__ __forceinline__ void table_insert(unsigned long long* tab_key, int* tab_mem, unsigned long long key, int r) {
  for (unsigned h = (unsigned)((key * kHashMul) >> 55), probe = 0; probe < (unsigned)kSlots; probe++, h = (h + 1u) & (kSlots - 1)) {
    const unsigned long long old = atomicCAS(&tab_key[h], 0ull, key);
    if (old == 0ull) { tab_mem[h] = r; break; }
    if (old == key) break;
  }
}

// ---- the phases of a streaming call, compiled into the ST instances only ----
// What the row says before a chunk of Tc frames: the frames consumed so far (a fresh row: 0, resume = false) or a status < 0;
// n: the members to resume with.  The same for every thread of the workgroup (returned wave-uniform).
template <bool LM>
__device__ __forceinline__ int asg_stream_open(const AsgBeamParams& p, const AsgStream& sp, const unsigned char* row, int Tc,
                                               bool& resume, int& n) {
  const AsgStreamHeader h = *reinterpret_cast<const AsgStreamHeader*>(row);
  int st = 0, res = 0, nn = 1;
  if (h.magic != 0u) {
    const bool same = h.magic == kAsgStreamMagic && h.V == p.V && h.R == p.R && h.W == p.W && h.has_lm == (LM ? 1 : 0) &&
                      h.max_frames == sp.max_frames && h.n >= 0 && h.n <= p.W && h.dead == (h.n == 0 ? 1 : 0) &&
                      h.frames >= 1 && h.frames <= sp.max_frames;
    if (same) { st = h.frames; res = 1; nn = h.n; } else st = kAsgStreamOtherConfig;
  }
  if (st >= 0 && st + Tc > sp.max_frames) st = kAsgStreamTooManyFrames;
  resume = __builtin_amdgcn_readfirstlane(res) != 0;
  n = __builtin_amdgcn_readfirstlane(nn);
  return __builtin_amdgcn_readfirstlane(st);
}

// The search of one utterance, whole (ST = false: the parameter block is AsgBeamParams and sp is not read) or streamed: one
// piece of source, and without ST the code the kernel had before it could stream, instruction for instruction
// (tools/diag/isa_compare.py).
// LEX (with LM): the search restricted to the model's lexicon.  TS: the read-out also writes the timesteps -- an instance of
// its own, because the plain read-out's walk (T dependent hops) must not pay for the division, nor the frames for a pointer
// more in scalar registers: without TS the code is the kernel's before there were timesteps, instruction for instruction.
// ST: resume from the state row, run the chunk's frames as frames f0 .. of the stream, suspend; the timesteps are then a
// run-time test on p.timesteps (TS is not read).
// CUT: the pruned search (e2e_asg_beam_nbest_cut, e2e_asg_beam_stream_cut; DESIGN.md 4.10, Pruned).  A frame expands the K
// labels of its list alone (written by launch_label_cut on the same stream): pair id is (m = id / K, c = kept[id - m * K]),
// a member whose last label is not kept has no stay candidate, and ctot / sval / spos hold W * K cells.  Without CUT the
// code the kernel had before, instruction for instruction (profiles/asg_cut/isa_identity.txt).
template <bool LM, bool LEX, bool TS, bool ST = false, bool CUT = false>
__global__ __launch_bounds__(kThreads) void asg_beam_kernel(AsgKernelParams<ST, CUT> q) {
  static_assert(LM || !LEX, "a restricted search has a model");
  const AsgBeamParams& p = beam_of(q);
  const AsgStream& sp = stream_of(q);
  using LmSet = typename std::conditional<LM, LmMembers, NoLm>::type;
  using CutSet = typename std::conditional<CUT, CutFrame, NoLm>::type;
  __shared__ Members mem[2];
  __shared__ LmSet lms[2];
  __shared__ CutSet cf;
  __shared__ double xs[kMaxV];
  __shared__ double ext[kMaxW];
  __shared__ unsigned long long tab_key[kSlots];
  __shared__ int tab_mem[kSlots];
  __shared__ BeamCut cut;
  __shared__ int n_surv, n_stay;
  __shared__ unsigned long long sh_floor;

  const int b = blockIdx.x, tid = threadIdx.x;
  const int V = p.V, W = p.W;
  const int PS = cut_pairs_of(q, V);                              // the pairs of a member: id = m * PS + (CUT: the place of) c
  const int64_t Tq = p.x_len[b];
  int Tb, f0 = 0, n_mem = 1;                                      // the frames to run, the stream's frames before them, the members
  bool resume = false;
  unsigned char* row = nullptr;
  if constexpr (ST) {
    row = sp.rows + (size_t)b * sp.row_bytes;
    Tb = Tq < 0 ? 0 : Tq > p.T ? p.T : (int)Tq;
    f0 = asg_stream_open<LM>(p, sp, row, Tb, resume, n_mem);
    // a status, or a fresh row fed nothing (the whole call on no frames): nothing of the row or the utterance is touched
    if (f0 < 0 || f0 + Tb == 0) {
      if (tid == 0) { sp.frames_done[b] = f0; if (p.nbest) p.n_hyp[b] = f0; }
      return;
    }
  } else {
    if (Tq < 1 || Tq > p.T) { if (tid == 0) p.n_hyp[b] = 0; return; }
    Tb = (int)Tq;
  }
  unsigned char* ws = p.ws + (size_t)b * p.per_utt;
  unsigned long long* ctot = reinterpret_cast<unsigned long long*>(ws);           // okey(total) per pair id, kNoCand: none
  unsigned long long* sval = reinterpret_cast<unsigned long long*>(ws + p.off_sval);
  int* spos = reinterpret_cast<int*>(ws + p.off_spos);
  int2* nodes = reinterpret_cast<int2*>(ST ? row + sp.off_nodes : ws + p.off_nodes);

  if (ST && resume) {                                             // the row's members become set 0
    stream_copy<kThreads>(&mem[0], row + kAsgStreamHeaderBytes, sizeof(Members));
    if constexpr (LM) stream_copy<kThreads>(&lms[0], row + sp.off_lm, sizeof(LmMembers));
  } else if (tid == 0) {
    mem[0].s[0] = 0.0; mem[0].key[0] = kKeyBasis; mem[0].last[0] = -1; mem[0].node[0] = 0; mem[0].len[0] = 0; mem[0].nw[0] = 0;
    if constexpr (LM) {
      LmMembers& L = lms[0];
      L.hash[0] = kFnvInit; L.lm[0] = 0.0; L.lmb[0] = 0.0; L.oov[0] = 0; L.oovb[0] = 0;
      for (int i = 0; i < kCtx; i++) { L.st[i][0] = 0u; L.stb[i][0] = 0u; }
      L.st[0][0] = p.lm.bos; L.stb[0][0] = p.lm.bos; L.stn[0] = 1; L.stbn[0] = 1;
    }
    nodes[0] = make_int2(-1, 0);
  }
  for (int i = tid; i < kSlots; i += kThreads) { tab_key[i] = 0ull; tab_mem[i] = -1; }
  __syncthreads();
  if constexpr (ST) {                                             // the table of the resumed members, as the step's last phase fills it
    if (resume && tid < n_mem) table_insert(tab_key, tab_mem, mem[0].key[tid], tid);
    __syncthreads();
  }

  int cur = 0;
  for (int t = 0; t < Tb && n_mem > 0; t++) {
    const Members& M = mem[cur];
    Members& N = mem[cur ^ 1];
    // ---- the frame's emissions; no member has an extension share yet ----
    {
      const int64_t row = (int64_t)b * p.sB + (int64_t)t * p.sT;
      for (int c = tid; c < V; c += kThreads) {
        const int64_t at = row + (int64_t)c * p.sV;
        xs[c] = p.dtype == E2E_F32 ? (double)reinterpret_cast<const float*>(p.x)[at] : reinterpret_cast<const double*>(p.x)[at];
      }
      if (tid < kMaxW) ext[tid] = ninf();
      if (tid == 0) { n_surv = 0; cut.n_sel = 0; n_stay = 0; sh_floor = ~0ull; }
      if constexpr (CUT) {
        // the frame's list (ascending) and the place of every label in it: thread i owns the labels above the list's entry
        // i - 1 up to its own, the last thread those behind it as well -- one writer per cell, no barrier of its own
        if (tid < PS) {
          const int32_t* lst = cut_ids_of(q) + ((int64_t)b * p.T + t) * PS;
          const int c = lst[tid];
          const int prev = tid > 0 ? lst[tid - 1] : -1;
          const bool ok = (unsigned)c < (unsigned)V;              // (always, for a list the selection wrote: no index leaves LDS)
          const int hi = tid == PS - 1 || !ok ? V : c;
          for (int j = (prev < -1 ? -1 : prev) + 1; j < hi; j++) cf.place_of[j] = -1;
          cf.kept[tid] = ok ? c : 0;
          if (ok) cf.place_of[c] = tid;
        }
      }
    }
    __syncthreads();
    // ---- every (member, label) pair: its share, and whom it goes to ----
    const int n_now = n_mem * PS;
    for (int id = tid; id < n_now; id += kThreads) {
      const int m = id / PS, c = label_at<CUT>(cf, id - m * PS);
      const int a = M.last[m];
      if (c == a) continue;                                       // the stay: below, once the extension shares are in
      unsigned long long cand = kNoCand;
      if (spellable(p, a, c)) {
        const double v = ext_mass(p, M, xs, m, a, c);
        const unsigned long long key = child_key(M.key[m], c);
        int hit = -1;
        for (unsigned h = (unsigned)((key * kHashMul) >> 55), probe = 0; probe < (unsigned)kSlots; probe++, h = (h + 1u) & (kSlots - 1)) {
          const unsigned long long k = tab_key[h];
          if (k == key) { hit = tab_mem[h]; break; }
          if (k == 0ull) break;
        }
        if (hit >= 0) ext[hit] = v;                               // (the only pair that spells member `hit`)
        else if (v > ninf()) {                                    // (false for NaN as well)
          const bool nwd = new_word(p, a, c);
          const int nw = M.nw[m] + (nwd ? 1 : 0);
          double lm = 0.0; int noov = 0;
          bool admissible = true;
          if constexpr (LM) {
            const LmMembers& L = lms[cur];
            if (c != p.space_id) {
              const LmAnswer ans = lm_query<LEX>(p, L, m, a, c, nwd);
              const ChildLm s = child_lm(L, m, nwd, ans);
              lm = s.lm; noov = s.oov;
              if constexpr (LEX) admissible = ans.listed;          // the last word, expanded, is spelled in Pref(L)
            } else {
              lm = L.lm[m]; noov = L.oov[m];
              // the space ends a word of L: the member's last lookup found an id, so it counted no OOV (a prefix has id 0)
              if constexpr (LEX) admissible = a < 0 || L.oov[m] == L.oovb[m];
            }
          }
          const double tot = total_of(p, v, lm, nw, noov);
          if (admissible && tot > ninf()) cand = okey(tot);
        }
      }
      ctot[id] = cand;
    }
    __syncthreads();
    // ---- the members' own candidates: stay and extension share together ----
    if (tid < n_mem) {
      const int m = tid, a = M.last[m];
      int at = a;                                                 // CUT: a's place in the list; not kept: no stay, no cell
      if constexpr (CUT) at = a >= 0 ? cf.place_of[a] : -1;
      if (at >= 0) {
        const double mass = stay_mass(p, M, xs, ext, m, a);
        double lm = 0.0; int noov = 0;
        if constexpr (LM) { lm = lms[cur].lm[m]; noov = lms[cur].oov[m]; }
        const double tot = total_of(p, mass, lm, M.nw[m], noov);
        unsigned long long cand = kNoCand;
        if (mass > ninf() && tot > ninf()) { cand = okey(tot); atomicMin(&sh_floor, cand); atomicAdd(&n_stay, 1); }
        ctot[m * PS + at] = cand;
      }
    }
    __syncthreads();
    // ---- an exact filter: a full beam's members are W candidates themselves, so nothing below the least of them can make
    //      the cut; what is left (usually a few times W) is what the selection reads ----
    const unsigned long long floor_bits = n_stay == W ? sh_floor : 1ull;
    for (int id = tid; id < n_now; id += kThreads) {
      const unsigned long long v = ctot[id];
      if (v < floor_bits) continue;                               // (kNoCand = 0 is below both)
      const int j = atomicAdd(&n_surv, 1);
      sval[j] = v; spos[j] = id;
    }
    __syncthreads();
    // ---- the cut: the W largest totals, exactly equal ones by ascending key ----
    beam_cut<kThreads>(cut, sval, spos, n_surv, W,
        [&](int id) { const int m = id / PS, c = label_at<CUT>(cf, id - m * PS); return c == M.last[m] ? M.key[m] : child_key(M.key[m], c); },
        okey_inv);
    // (the key table is the old members': every pair has looked its key up)
    for (int i = tid; i < kSlots; i += kThreads) { tab_key[i] = 0ull; tab_mem[i] = -1; }
    __syncthreads();
    const int ns = beam_cut_count(cut, W);
    if (ns == 0) { n_mem = 0; break; }                            // no candidate has a number for a total: no hypothesis is left
    // ---- rank the survivors: they become the members in that order ----
    beam_cut_rank(cut, ns);
    __syncthreads();
    if (tid < ns) {
      const int id = cut.sel_pos[tid], r = cut.sel_rank[tid];
      const int m = id / PS, c = label_at<CUT>(cf, id - m * PS), a = M.last[m];
      const unsigned long long key = cut.sel_key[tid];
      N.key[r] = key; N.last[r] = c;
      if (c == a) {                                               // the member stays
        N.s[r] = stay_mass(p, M, xs, ext, m, a);
        N.node[r] = M.node[m]; N.len[r] = M.len[m]; N.nw[r] = M.nw[m];
        if constexpr (LM) copy_lm(lms[cur ^ 1], r, lms[cur], m);
      } else {                                                    // a new sequence: member m's, and label c
        N.s[r] = ext_mass(p, M, xs, m, a, c);
        const int node = 1 + (ST ? f0 + t : t) * W + r;           // (the frame of the stream, not of the chunk)
        nodes[node] = make_int2(M.node[m], c);
        N.node[r] = node; N.len[r] = M.len[m] + 1;
        const bool nwd = new_word(p, a, c);
        N.nw[r] = M.nw[m] + (nwd ? 1 : 0);
        if constexpr (LM) {                                        // get_next_prefix's LM part, as ctc_beam.hip's child_lm
          const LmMembers& L = lms[cur]; LmMembers& O = lms[cur ^ 1];
          if (c != p.space_id) {
            const LmAnswer ans = lm_query(p, L, m, a, c, nwd);
            const ChildLm s = child_lm(L, m, nwd, ans);
            int bn = nwd ? L.stn[m] : L.stbn[m];
            O.stbn[r] = bn;
#pragma unroll
            for (int i = 0; i < kCtx; i++) O.stb[i][r] = nwd ? L.st[i][m] : L.stb[i][m];
            O.lmb[r] = s.lmb; O.oovb[r] = s.oovb;
            if (bn > p.lm.order - 1) bn = p.lm.order - 1;
            int sn = bn + 1; if (sn > p.lm.order - 1) sn = p.lm.order - 1;
#pragma unroll
            for (int i = kCtx - 1; i >= 1; i--) O.st[i][r] = i < sn ? O.stb[i - 1][r] : 0u;
            O.st[0][r] = sn > 0 ? ans.wi : 0u;
            O.stn[r] = sn;
            O.hash[r] = ans.h;
            O.lm[r] = s.lm; O.oov[r] = s.oov;
          } else copy_lm(O, r, L, m);                             // a space copies the fields
        }
      }
      table_insert(tab_key, tab_mem, key, r);
    }
    n_mem = ns; cur ^= 1;
    __syncthreads();
  }

  // ---- suspend, behind the chunk's last frame: the current set, then the header.  A chunk of no frames stores nothing ----
  if constexpr (ST) {
    if (Tb > 0) {
      stream_copy<kThreads>(row + kAsgStreamHeaderBytes, &mem[cur], sizeof(Members));
      if constexpr (LM) stream_copy<kThreads>(row + sp.off_lm, &lms[cur], sizeof(LmMembers));
    }
    if (tid == 0) {
      if (Tb > 0) {
        AsgStreamHeader h;
        h.magic = kAsgStreamMagic; h.V = V; h.R = p.R; h.W = W; h.has_lm = LM ? 1 : 0; h.max_frames = sp.max_frames;
        h.n = n_mem; h.frames = f0 + Tb; h.dead = n_mem == 0 ? 1 : 0;
        *reinterpret_cast<AsgStreamHeader*>(row) = h;
      }
      sp.frames_done[b] = f0 + Tb;
    }
    if (p.nbest == 0) return;                                     // feed only
  }

  // ---- read-out: the first nbest members, ranked already ----
  const Members& F = mem[cur];
  const int nbest = p.nbest;
  const int64_t max_out = p.max_out;
  const bool want_ts = ST ? p.timesteps != nullptr : TS;
  const int max_hops = ST ? f0 + Tb : p.T;                        // a sequence has at most one node per frame consumed
  int64_t* out = p.out + (int64_t)b * nbest * max_out;
  int64_t* ts = nullptr;
  if (want_ts) ts = p.timesteps + (int64_t)b * nbest * max_out;
  __syncthreads();
  if (tid < nbest) {
    int64_t* row = out + (int64_t)tid * max_out;
    int64_t* trow = nullptr;
    if (want_ts) trow = ts + (int64_t)tid * max_out;
    int len = 0, nw = 0, noov = 0;
    double ac = ninf(), lm = 0.0, tot = ninf();
    if (tid < n_mem) {
      len = F.len[tid]; ac = F.s[tid]; nw = F.nw[tid];
      if constexpr (LM) { lm = lms[cur].lm[tid]; noov = lms[cur].oov[tid]; }
      tot = total_of(p, ac, lm, nw, noov);
      int at = len, node = F.node[tid];
      for (int hops = 0; node > 0 && hops <= max_hops; hops++) {
        if constexpr (ST) { if (node > W * sp.max_frames) break; }  // (no node of this row's pool: the row is not this call's)
        const int2 nd = nodes[node];
        --at;
        if (at >= 0 && at < max_out) {
          row[at] = (int64_t)nd.y;
          if (want_ts) trow[at] = (int64_t)((node - 1) / W);        // node = 1 + t * W + rank
        }
        node = nd.x;
      }
    }
    cut.sel_pos[tid] = len;
    const int64_t o = (int64_t)b * nbest + tid;
    p.out_len[o] = len;
    p.scores[o * 3 + 0] = tot; p.scores[o * 3 + 1] = ac; p.scores[o * 3 + 2] = lm;
    p.counts[o * 2 + 0] = nw; p.counts[o * 2 + 1] = noov;
  }
  __syncthreads();
  for (int j = 0; j < nbest; j++) {
    int64_t* row = out + (int64_t)j * max_out;
    for (int64_t i = cut.sel_pos[j] + tid; i < max_out; i += kThreads) row[i] = 0;
    if (want_ts) for (int64_t i = cut.sel_pos[j] + tid; i < max_out; i += kThreads) ts[(int64_t)j * max_out + i] = -1;
  }
  if (tid == 0) p.n_hyp[b] = n_mem < nbest ? n_mem : nbest;
}

// the transitions as the search reads them: f64, [from][to]; all zero without a matrix
__global__ void asg_beam_transpose_kernel(const void* A, int dtype, int V, double* At) {
  const int n = V * V;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int from = i / V, to = i - from * V;
    double v = 0.0;
    if (A) v = dtype == E2E_F32 ? (double)reinterpret_cast<const float*>(A)[to * V + from] : reinterpret_cast<const double*>(A)[to * V + from];
    At[i] = v;
  }
}

struct Layout { size_t head, per_utt, off_sval, off_spos, off_nodes; };

// PS: the pairs of a member, V (0) or a pruned call's K
bool layout(int T, int V, int W, Layout& L, int PS = 0) {
  if (T < 1 || V < 1 || V > kMaxV || W < 1 || W > kMaxW || W * V > kMaxPairs || T > (1 << 22) || PS < 0 || PS > V) return false;
  const size_t ids = (size_t)W * (PS ? PS : V);
  L.head = align_up((size_t)V * V * 8, 256);
  size_t at = align_up(ids * 8, 256);
  L.off_sval = at; at += align_up(ids * 8, 256);
  L.off_spos = at; at += align_up(ids * 4, 256);
  L.off_nodes = at; at += align_up(((size_t)W * ((size_t)T + 1) + 1) * 8, 256);
  L.per_utt = at;
  return true;
}

// a state row of a stream: header | Members | LmMembers (with a model) | node pool of max_frames frames, each 256-aligned
struct StreamLayout { size_t off_lm, off_nodes, total; };
bool stream_layout(int max_frames, int V, int W, bool lm, StreamLayout& S) {
  Layout L;
  if (max_frames < 1 || !layout(max_frames, V, W, L)) return false;
  S.off_lm = kAsgStreamHeaderBytes + align_up(sizeof(Members), 256);
  S.off_nodes = S.off_lm + (lm ? align_up(sizeof(LmMembers), 256) : 0);
  S.total = S.off_nodes + align_up(((size_t)W * ((size_t)max_frames + 1) + 1) * 8, 256);
  return true;
}

// the model's argument errors, the whole call's and the stream's: what the host sees without a HIP call ...
int check_model(const e2e_lm* lm, int V, bool restricted) {
  if (lm) {
    if (lm->transcribed) {
      set_error("the ASG search spells its words from the labels' strings: a model with custom transcriptions (e2e_lm_load_transcriptions) is not supported");
      return E2E_ERR_UNSUPPORTED;
    }
    if (lm->order > kLmMaxOrder) { set_error("a language model of order %d: at most %d", lm->order, kLmMaxOrder); return E2E_ERR_UNSUPPORTED; }
    if ((int)lm->label_off.size() - 1 != V) {
      set_error("the language model was loaded with %d labels but the emissions have %d columns", (int)lm->label_off.size() - 1, V);
      return E2E_ERR_ARG;
    }
  }
  return check_lexicon(lm, restricted);
}
// (... and the device its tables are on: check_model_device, ctc_lm.h)

// every argument error that the whole call (min_nbest = 1) and the stream (0: feed only) have in common, in the order they are
// reported; without a read-out max_out is not looked at
int check_beam_args(int dtype, int B, int T, int V, int num_replabels, int space_id, int beam_width, int nbest, int64_t max_out,
                    int min_nbest = 1) {
  if (dtype != E2E_F32 && dtype != E2E_F64) { set_error("dtype must be E2E_F32 or E2E_F64"); return E2E_ERR_ARG; }
  if (B < 0 || T < 1 || V < 1 || ((min_nbest > 0 || nbest > 0) && max_out < 0)) {
    set_error("bad sizes B=%d T=%d V=%d max_out=%lld", B, T, V, (long long)max_out); return E2E_ERR_ARG;
  }
  if (V > e2e_asg_max_labels()) { set_error("V=%d exceeds e2e_asg_max_labels() = %d", V, e2e_asg_max_labels()); return E2E_ERR_UNSUPPORTED; }
  if (num_replabels < 0 || num_replabels >= V) { set_error("num_replabels=%d outside [0, V=%d)", num_replabels, V); return E2E_ERR_ARG; }
  if (space_id >= V - num_replabels) { set_error("space_id=%d is not one of the %d characters", space_id, V - num_replabels); return E2E_ERR_ARG; }
  if (beam_width < 1) { set_error("beam_width %d must be at least 1", beam_width); return E2E_ERR_ARG; }
  if (beam_width > e2e_asg_beam_max_width(V)) {
    set_error("beam_width %d exceeds e2e_asg_beam_max_width(V=%d) = %d", beam_width, V, e2e_asg_beam_max_width(V));
    return E2E_ERR_UNSUPPORTED;
  }
  if (nbest < min_nbest || nbest > beam_width) { set_error("nbest=%d outside [%d, beam_width=%d]", nbest, min_nbest, beam_width); return E2E_ERR_ARG; }
  return E2E_OK;
}

// the search's parameter block, the whole call's and the stream's alike; where the nodes lie (per_utt, off_nodes) is the caller's
void fill_params(AsgBeamParams& p, const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len, int B, int T,
                 int V, int num_replabels, int beam_width, int space_id, const e2e_lm* lm, double lmwt, double wip,
                 double oov_penalty, int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp, double* scores,
                 int32_t* counts, int64_t* timesteps, void* workspace, const Layout& L, size_t per_utt, size_t off_nodes) {
  p.x = x; p.dtype = dtype; p.sB = sB; p.sT = sT; p.sV = sV; p.x_len = x_len;
  p.B = B; p.T = T; p.V = V; p.R = num_replabels; p.W = beam_width; p.space_id = space_id < 0 ? -1 : space_id; p.nbest = nbest;
  if (lm) p.lm = lm->dev_view(); else memset(&p.lm, 0, sizeof(p.lm));
  p.lmwt = lm ? lmwt : 0.0; p.wip = wip; p.oov = oov_penalty;
  p.out = out; p.max_out = max_out; p.out_len = out_len; p.n_hyp = n_hyp; p.scores = scores; p.counts = counts;
  p.timesteps = timesteps;
  unsigned char* base = reinterpret_cast<unsigned char*>(workspace);
  p.At = reinterpret_cast<const double*>(base);
  p.ws = base + L.head; p.per_utt = per_utt; p.off_sval = L.off_sval; p.off_spos = L.off_spos; p.off_nodes = off_nodes;
}

// the transitions into the head of the workspace, then the search: q is the kernel's parameter block, p the search's in it
template <typename Kernel, typename Params>
int launch(Kernel kernel, const Params& q, const AsgBeamParams& p, const void* transitions, void* stream, const char* what) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(asg_beam_transpose_kernel, dim3((p.V * p.V + 255) / 256), dim3(256), 0, s, transitions, p.dtype, p.V,
                     const_cast<double*>(p.At));
  E2E_HIP_CHECK(hipGetLastError(), "asg_beam_transpose_kernel launch");
  hipLaunchKernelGGL(kernel, dim3(p.B), dim3(kThreads), 0, s, q);
  E2E_HIP_CHECK(hipGetLastError(), what);
  return E2E_OK;
}

}  // namespace
}  // namespace e2e
