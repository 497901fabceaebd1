// Prefix beam search (Hannun et al. 2014) with optional n-gram LM scoring, on the GPU.
// Restates src/decoders/ctc_decoder.cpp:153-201 (driver), :353-441 (decode_sentence), :247-312
// (get_next_prefix), :314-318 (score), :232-245 (get_sentence).
//
// One 1024-thread workgroup per utterance; time is serial, the W*V (prefix, character) pairs of a step are
// spread over the threads.  The prefix tree lives in a per-utterance node pool in HBM (parent, character: written once,
// read only for the final sentence).  The reference's shared_ptr / weak_ptr ownership -- a prefix lives while it is in
// the beam or has a living child; the weak `next_data` entry of its parent expires when it dies -- is restated without
// reference counts:
//   * only beam members are ever asked for a child, so what has to be known is, for every member P and character c,
//     whether the child (P, c) is alive, i.e. is a member or an ancestor of one (a pruned child that is kept alive by
//     a descendant is still found, receives probability that nobody reads, and is NOT re-added: quirk Q7);
//   * every member j carries its GUARD: the first prefix on its way to the root (itself included) whose parent is a
//     member, as (owner = that parent's position in the beam, character, node id).  Every alive child of a member is
//     the guard of some member (of itself, if it is one), so the members' child tables are REBUILT each step from the
//     guards: cleared, then one LDS write per member.  When a guard's owner leaves the beam, the guard is inherited
//     from the owner's own guard (the next alive prefix up the path whose parent is still a member).
//   No global atomics, no reads of the node pool inside the step loop.
// All scores are IEEE doubles with the reference's two-argument log-sum-exp.  The beam (probabilities, LM state, child
// tables) lives in LDS; prefixes are created LAZILY: a step scores all W*V would-be prefixes, selects the W survivors
// (radix select on an order-preserving 64-bit key started below the bits the best and the worst surviving score share --
// one pass in practice -- then a rank-by-counting of the <= W+63 gathered candidates into (score descending, position
// ascending) order: the reference's nth_element leaves ties unspecified, quirk Q9; the oracle uses the same total order)
// and only then allocates nodes for the new ones.  Upstream a new prefix that does not survive its first pruning is
// destroyed at once, so this is equivalent and saves ~W*V allocations, LM-state writes and frees per step.
//
// The language model stands where KenLM stands upstream (src/decoders/ctc_decoder.cpp:60-71,77-88,264-308):
// host-side ARPA reader (plain or gzip, ctc_lm.hip), device-resident open-addressing tables (ctc_lm.h), standard back-off
// scoring.  A beam
// member's V answers are looked up once per LM state when it enters the beam and kept in LDS (see lm_query).
//
// Two read-outs end the search: read_out() -- the best prefix's sentence, what upstream's sort + [0] keeps (e2e_ctc_beam) -- and
// read_out_nbest() -- the first `nbest` of the ranked final beam with their scores, counts and, if asked for, the frame at which
// each label's prefix was created (e2e_ctc_beam_nbest; no counterpart upstream).
//
// The search can stop after any frame and go on in a later launch (e2e_ctc_beam_stream): what a step hands to the next -- one
// member set, the member count, the node pool and its counter -- is kept in a state row in HBM, everything else is rebuilt
// at resume (StreamHeader, stream_open / stream_load_members / stream_suspend; the kernels' ST instances).
//
// This header is what the two kernels and the host side share: the types, the constants, the LM queries and the phases both
// kernels run (all __forceinline__: every kernel instance carries its own copy, none is a function of its own).
//   ctc_beam_lds.hip      ctc_beam_kernel: the beam in LDS                   } each compiled once per input dtype
//   ctc_beam_general.hip  ctc_beam_general_kernel: any alphabet width        } (-DE2E_BEAM_IO=<type>), 18 instances an object
//                         ... and once more per dtype for the pruned calls (-DE2E_BEAM_CUT=true; per-frame label pruning)
//   ctc_label_cut.hip     label_cut_kernel: which labels of a frame a pruned call expands
//   ctc_beam.hip          the host side: layouts, kernel choice, the C entry points
// A kernel object hands its instances out through lds_kernel<IO> / general_kernel<IO, CUT> below.
#pragma once
#include "beam_cut.h"
#include "ctc_lm.h"

namespace e2e {
namespace beamk {

constexpr int kThreads = 1024;     // (with a language model: 512 threads measured 30 % slower)
constexpr int kMaxCand = 8192;     // W*V + W candidates per step (LDS key array)
constexpr int kLdsBudget = 158 * 1024;
constexpr int kSelBits = 11, kSelBins = 1 << kSelBits;   // radix-select digit (two alternating histograms in LDS)
constexpr int kStateSlots = 512;                       // LM state table of a step (open addressing, <= half full: checked by the host)
constexpr int kSelSmall = 64;                           // a threshold bin this small is finished exactly by one wave

// LM-related state of a prefix (Prefix::lm_*, num_*, last_word, ctc_decoder.h:79-86)
struct LmFields {
  double lm_score, lm_before;
  int num_words, num_oov, num_oov_before, word_len;
  unsigned long long word_hash;            // hash of the spelled last word (get_idx(vector<int>), :84-88)
  unsigned int st[kCtx], stb[kCtx];        // LM context after / before the last word, most recent first
  int st_n, stb_n;
};

// tree node in HBM: the structure only (8 bytes).  Everything a prefix needs while it is in the beam -- the four
// log-probabilities, the LM state, its child table, its parent's id -- lives in LDS; a pruned-but-alive prefix still
// "receives" probability upstream, but nothing ever reads it: quirk Q7 reduces to "its (parent, char) slot stays
// occupied".  Nodes are never reused: at most W prefixes are created per step, so W*(T+3) nodes cover an utterance
// and allocation is a counter (no free list to initialise, read or write).
struct BeamNode {
  int parent, last_char;
};

struct BeamParams {
  const void* lp; int64_t sB, sT, sV; const int64_t* x_len;
  int B, T, V, blank, W, space_id;
  int has_lm; LmView lm; double lmwt, wip, oov;
  int64_t* out; int64_t max_out; int64_t* out_len;
  BeamNode* nodes;                                    // per-utterance workspace
  int NCAP, CMAX, WP2, HS;
  // The n-best read-out (e2e_ctc_beam_nbest).  nbest == 0 is the plain call: read_out() runs and none of the rest is read.
  int nbest;
  int64_t* n_hyp; double* scores; int* counts;        // (B), (B,nbest,3), (B,nbest,2); out / out_len are (B,nbest,max_out) / (B,nbest)
  int64_t* ts_out;                                    // (B,nbest,max_out) frames of the output ids, or null
  int* node_t;                                        // [B][NCAP] beside `nodes`: the frame at which a node was created.  Null unless
                                                      // timestamps were asked for: the step loop then stores nothing more
  // The streaming call (e2e_ctc_beam_stream: the kernels' ST instances).  Every other call reads nothing below.  x_len is the
  // chunk's lengths, T its width, NCAP the pool of st_max_frames frames; nodes / node_t above are not used (they live in the row).
  unsigned char* st_rows; size_t st_row_bytes;        // (B, row_bytes): one self-contained state row per utterance (StreamHeader)
  size_t st_nodes_off, st_ts_off;                     // the node pool and the nodes' frames inside a row (st_ts_off 0: not kept)
  int st_max_frames;
  int64_t* frames_done;                               // (B): frames consumed so far, or the in-band status
};

// ---- the state row of a stream: header (256 bytes), one member set, the node pool, the nodes' frames ----
// The row holds indices only (node ids, positions in the beam, word ids), never an address: it may be moved or copied.
// magic == 0 -- what a zeroed header has -- is a fresh utterance.  Of a member set everything that survives a step is kept
// (probabilities, `full`, node, last character, guard, LM state; inc / kept in the state the rebuild leaves them in); what a
// step rebuilds is not: the slot map, the child tables (from the guards) and the LM's answers, which are a function of a
// member's LM state alone and are asked again at resume -- 8 * W * V bytes that would make the row depend on the alphabet
// (6.4 MB at W = 100, V = 8000, against the 18 KB of the member set) for W * V look-ups per chunk, what a few steps ask anyway.
// A status (node pool exhausted, too many frames, another configuration) stores nothing, so a stored row carries no error flag.
constexpr unsigned kStreamMagic = 0x42533443u;
constexpr int kStreamHeaderBytes = 256;
struct StreamHeader {
  unsigned magic;
  int V, W, has_lm, max_frames, with_ts;              // the configuration the row was written under
  int n, next_node, frames;                           // members, nodes allocated, frames consumed
};
static_assert(sizeof(StreamHeader) <= kStreamHeaderBytes, "stream header");
constexpr int kStreamPoolExhausted = -1, kStreamTooManyFrames = -2, kStreamOtherConfig = -3;

// inclusive prefix sum over the 64 lanes, all DPP (row_shr 1/2/4/8 with zero fill, row_bcast 15/31)
__device__ __forceinline__ int wave_scan_i(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
  return v;
}

// maximum over the 64 lanes, all DPP; every lane of row 3 (lanes 48..63) ends with it, returned wave-uniform
// (the same function as lattice_common.h's wave_max_i: that header carries the lattice kernels' host code, so it is not included here)
__device__ __forceinline__ int wave_max_i(int v) {
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xf, 0xf, false));   // row_half_mirror
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xf, 0xf, false));   // row_mirror
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x142, 0xa, 0xf, false));   // row_bcast:15
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x143, 0xc, 0xf, false));   // row_bcast:31
  return __builtin_amdgcn_readlane(v, 63);
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for the wave's outstanding GLOBAL
// operations (vmcnt(0)), which would expose a memory round trip at every phase that follows a fire-and-forget store or
// the prefetch of the next row.  Two full barriers per step remain: after the rebuild (node stores and reference-count
// atomics before the release) and at the end of the step.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Candidate d >= n of a step is the pair q = d - n (q = c*n + i, the reference's order); a pair that creates no prefix
// holds this marker instead of a score: a negative NaN, which the order-preserving key maps BELOW -inf (scores can
// be -inf), and which every pass over the keys skips.
constexpr unsigned long long kNoCandKey = ~0xFFF8000000000000ULL;
// (the keys are beam_cut.h's okey: larger score <=> larger key)

// the LM part of get_next_prefix (:258-308) for the child (parent pr, char c)
// What a (prefix, character != space) pair asks of the language model: the id of the word spelled so far and its
// score in the prefix's context.  The answer depends on the prefix's LM state and the character only -- not on the time
// step -- so a beam member's V answers are looked up ONCE, when it enters the beam, by V different threads, and kept
// in LDS while it stays (`lmc`): the pair loop and the rebuild then read them instead of walking the n-gram tables
// (global memory, several dependent probes) for every pair of every step.
struct LmAnswer { float sc; uint32_t wi; };
// (LabelTab: the labels' spellings, staged in LDS by the kernel when they fit -- two dependent global loads less per query)
// (one: LDS, per label its byte -- case already folded -- if it is spelled with exactly one, else -1; null when not staged.
//  The usual alphabet: one LDS read instead of three dependent loads through generic pointers.)
struct LabelTab { const int* off; const unsigned char* bytes; const int* one; };
constexpr int kLabelLdsBytes = 512;
__device__ __forceinline__ unsigned long long spell(const BeamParams& p, const LabelTab& lt, unsigned long long h, int c) {
  if (lt.one) { const int o = lt.one[c]; if (o >= 0) return fnv_step(h, (unsigned char)o); }
  for (int bi = lt.off[c]; bi < lt.off[c + 1]; bi++) {
    unsigned char ch = lt.bytes[bi];
    if (p.lm.fold_case && ch >= 'A' && ch <= 'Z') ch += 32;
    h = fnv_step(h, ch);
  }
  return h;
}
// lm_base_score for contexts of up to kParCtx words in two rounds of table probes.  Round 1 (issued by the caller beside the
// vocabulary probe, which it does not depend on): the context k-grams -- their back-off weights and continuation bits.
// Round 2, once the word is known: the unigram, and the (k+1)-grams (ctx[k-1..0], word) whose context lists the word among
// its continuations.  Within a round every lookup that is still open requests its next slot before any answer is consumed.
// The answers are combined in the chain's order (same float additions as lm_base_score).
constexpr int kParCtx = 2;
struct LmContexts { float backoff[kParCtx + 1]; uint64_t cont[kParCtx + 1]; unsigned hit; uint64_t hp[kParCtx + 1]; };
__device__ __forceinline__ void lm_contexts(const LmView& lm, const uint32_t (&ctx)[kCtx], int n, LmContexts& cx) {
  const uint4* tab = reinterpret_cast<const uint4*>(lm.ngs);
  uint64_t h[kParCtx + 1]; uint32_t idx[kParCtx + 1]; uint4 e[kParCtx + 1];
  unsigned open = 0;
  cx.hit = 0; cx.hp[0] = kFnvInit;
#pragma unroll
  for (int k = 1; k <= kParCtx; k++) {
    uint64_t hp = kFnvInit;
#pragma unroll
    for (int i = 0; i < k; i++) hp = ng_mix(hp, ctx[k - 1 - i]);
    cx.hp[k] = hp;
    h[k] = ng_finish(hp, k);
    idx[k] = (uint32_t)h[k] & lm.ngmask;
    cx.backoff[k] = 0.f; cx.cont[k] = 0;
    if (k >= 2 && k <= n) { open |= 1u << k; e[k] = tab[2 * (size_t)idx[k]]; }
  }
  if (n >= 1) {                                   // the one-word context: the unigram entry itself
    const uint4 u = reinterpret_cast<const uint4*>(lm.uni)[ctx[0] < lm.nwords ? ctx[0] : 0];
    if (__uint_as_float(u.x) <= 0.f && ctx[0] < lm.nwords) {
      cx.hit |= 2u; cx.backoff[1] = __uint_as_float(u.y); cx.cont[1] = ((uint64_t)u.w << 32) | u.z;
    }
  }
  while (open) {
#pragma unroll
    for (int k = 2; k <= kParCtx; k++) {
      if (open >> k & 1u) {
        const uint64_t sig = ((uint64_t)e[k].y << 32) | e[k].x;
        if (sig == h[k]) {
          cx.hit |= 1u << k; open &= ~(1u << k);
          cx.backoff[k] = __uint_as_float(e[k].w);
          const uint4 c = tab[2 * (size_t)idx[k] + 1];                  // (same cache line as the slot's first half)
          cx.cont[k] = ((uint64_t)c.y << 32) | c.x;
        } else if (sig == 0) open &= ~(1u << k);
        else { idx[k] = (idx[k] + 1) & lm.ngmask; e[k] = tab[2 * (size_t)idx[k]]; }
      }
    }
  }
}
__device__ __forceinline__ float lm_score_parallel(const LmView& lm, const LmContexts& cx, int n, uint32_t word, float uni_prob) {
  const uint4* tab = reinterpret_cast<const uint4*>(lm.ngs);
  uint64_t h[kParCtx + 1]; uint32_t idx[kParCtx + 1]; uint4 e[kParCtx + 1];
  float prob[kParCtx + 1];
  unsigned open = 0, hit = 0;
  const int bit = cont_bit(word);
#pragma unroll
  for (int k = 0; k <= kParCtx; k++) {
    h[k] = ng_finish(ng_mix(cx.hp[k], word), k + 1);
    idx[k] = (uint32_t)h[k] & lm.ngmask;
    prob[k] = 0.f;
    // (only if the context is listed and lists the word among its continuations)
    if (k >= 1 && k <= n && (cx.hit >> k & 1u) && (cx.cont[k] >> bit & 1ULL)) { open |= 1u << k; e[k] = tab[2 * (size_t)idx[k]]; }
  }
  if (uni_prob <= 0.f) { hit |= 1u; prob[0] = uni_prob; }          // (the unigram came with the vocabulary entry)
  while (open) {
#pragma unroll
    for (int k = 1; k <= kParCtx; k++) {
      if (open >> k & 1u) {
        const uint64_t sig = ((uint64_t)e[k].y << 32) | e[k].x;
        if (sig == h[k]) { hit |= 1u << k; open &= ~(1u << k); prob[k] = __uint_as_float(e[k].z); }
        else if (sig == 0) open &= ~(1u << k);
        else { idx[k] = (idx[k] + 1) & lm.ngmask; e[k] = tab[2 * (size_t)idx[k]]; }
      }
    }
  }
  // longest listed n-gram, then the back-off weights of the longer contexts, shortest first (KenLM's float order)
  int found_k = 0;
  float result = lm.unk_prob;
#pragma unroll
  for (int k = 0; k <= kParCtx; k++)
    if (k <= n && (hit >> k & 1u)) { result = prob[k]; found_k = k; }
#pragma unroll
  for (int k = 1; k <= kParCtx; k++)
    if (k > found_k && k <= n && (cx.hit >> k & 1u)) result += cx.backoff[k];
  return result;
}
// The search restricted to the model's lexicon (e2e_ctc_beam_opts.restrict_to_lexicon; the definition is in DESIGN.md 4.4):
// a child is created only if its word's spelling is a word of the lexicon or a prefix of one, and a space only behind a
// whole word.  The vocabulary tables of a model with a lexicon list the prefixes that are no words with id 0, so the probe
// that finds the word's id also answers the first question: a spelling that is not in the table at all gets kNoChildWord
// for an answer, and the pair loop creates no candidate for it.  The second follows from what a member holds already.
constexpr uint32_t kNoChildWord = 0xFFFFFFFFu;
// LMK, the kernels' template argument: 0 no language model, 1 the general LM walk, 2 the fast one (see lm_query); 3 and 4 are
// 1 and 2 restricted to the lexicon (instances of their own: the unrestricted ones carry nothing of the rule); 5 to 8 are 1 to 4
// for a model with homophones (custom transcriptions; instances of their own again: as a branch on the mark inside 1 to 4 the
// second copy of the LM walk cost the fast instances their last free registers -- 12 to 20 bytes of scratch where there were none)
__host__ __device__ constexpr int lmk_base(int lmk) { return lmk > 4 ? lmk - 4 : lmk; }
__host__ __device__ constexpr bool lmk_fast(int lmk) { return lmk_base(lmk) == 2 || lmk_base(lmk) == 4; }
__host__ __device__ constexpr bool lmk_restricted(int lmk) { return lmk_base(lmk) >= 3; }
__host__ __device__ constexpr bool lmk_hom(int lmk) { return lmk > 4; }
// ... and the way back, what the host asks for: the instance of a call (fast, restricted, hom mean nothing without a model)
constexpr int kLmKinds = 9;
constexpr int lmk_of(bool lm, bool fast, bool restricted, bool hom) {
  return !lm ? 0 : 1 + (fast ? 1 : 0) + (restricted ? 2 : 0) + (hom ? 4 : 0);
}
constexpr bool lmk_of_inverts_the_decoders() {
  for (int k = 0; k < kLmKinds; k++)
    if (lmk_of(k != 0, lmk_fast(k), lmk_restricted(k), lmk_hom(k)) != k) return false;
  return true;
}
static_assert(lmk_of_inverts_the_decoders(), "lmk_of must be the inverse of lmk_fast / lmk_restricted / lmk_hom for all nine codes");
// FAST: the model has signature tables and at most kParCtx words of context (checked by the host): only the round-probed
// walk is compiled in.  Otherwise: the general walk over the id tables (any order up to 6).
// HOM: the model has homophone sets (ctc_lm.h): a marked table value is resolved by scoring every word of its set.
template <bool FAST, bool RS, bool HOM>
__device__ __forceinline__ LmAnswer lm_query(const BeamParams& p, const LabelTab& lt, const LmFields& pr, int parent_last, int c) {
  const bool new_word = pr.num_words == 0 || parent_last == p.space_id;                           // :258-259 (c != space)
  LmAnswer a;
  uint64_t h = spell(p, lt, new_word ? kFnvInit : pr.word_hash, c);

  int cn = new_word ? pr.st_n : pr.stb_n;
  if (FAST) {
    uint32_t ctx[kCtx];
#pragma unroll
    for (int s2 = 0; s2 < kCtx; s2++) ctx[s2] = new_word ? pr.st[s2] : pr.stb[s2];
    if (h == 0) h = 1;
    if (cn > p.lm.order - 1) cn = p.lm.order - 1;
    uint32_t v1, v2;
    two_slots(h, p.lm.vmask, v1, v2);
    const uint4 e1 = reinterpret_cast<const uint4*>(p.lm.vt)[v1], e2 = reinterpret_cast<const uint4*>(p.lm.vt)[v2];   // (in flight beside the context lookups)
    LmContexts cx;
    lm_contexts(p.lm, ctx, cn, cx);
    const bool in1 = (((uint64_t)e1.y << 32) | e1.x) == h, in2 = (((uint64_t)e2.y << 32) | e2.x) == h;
    if (RS && !in1 && !in2) { a.wi = kNoChildWord; a.sc = 0.f; return a; }
    a.wi = in1 ? e1.z : in2 ? e2.z : 0u;                             // NotFound() == <unk> == 0
    const float uni_prob = in1 ? __uint_as_float(e1.w) : in2 ? __uint_as_float(e2.w) : p.lm.unk_prob;
    if (HOM && is_hom_ref(a.wi)) {
      // homophones (a model with custom transcriptions): the word of this key is the one the model scores highest in this
      // context, exact ties to the earliest listed.  The contexts are looked up already; one round of probes per candidate.
      const uint32_t* set = p.lm.homs + (a.wi & ~kHomMark);
      const uint32_t count = set[0];
      a.sc = -INFINITY;
      for (uint32_t i = 0; i < count; i++) {
        const uint32_t w = set[1 + i];
        const float sc = lm_score_parallel(p.lm, cx, cn, w, p.lm.uni[w].prob);
        if (i == 0 || sc > a.sc) { a.sc = sc; a.wi = w; }
      }
      return a;
    }
    a.sc = lm_score_parallel(p.lm, cx, cn, a.wi, uni_prob);
  } else {
    if (RS) {
      if (!lm_word_find(p.lm, h, a.wi)) { a.wi = kNoChildWord; a.sc = 0.f; return a; }
    } else {
      a.wi = lm_word_lookup(p.lm, h);
    }
    if (HOM && is_hom_ref(a.wi)) { a.wi = lm_homophone_choice(p.lm, a.wi, new_word ? pr.st : pr.stb, cn, &a.sc); return a; }
    a.sc = lm_base_score(p.lm, new_word ? pr.st : pr.stb, cn, a.wi, nullptr, nullptr);
  }
  return a;
}

// restricted to the lexicon: is the child (member pr, character c) one that may not be created?  (pr: score_fields)
__device__ __forceinline__ bool lexicon_forbids(const BeamParams& p, const LmFields& pr, int parent_last, int c, LmAnswer ans) {
  // a space: only behind a whole word -- the member ends inside a word, and that word is not out of vocabulary
  if (c == p.space_id) return parent_last >= 0 && parent_last != p.space_id && pr.num_oov != pr.num_oov_before;
  return ans.wi == kNoChildWord;
}

// Quirk Q8's division, (double)score / ln 10, without the division: for every float whose magnitude lies in [2^-60, 2^20)
// -- all 671 088 640 of them checked against the IEEE quotient on the host (both signs are symmetric) -- the product with the
// rounded reciprocal, corrected once through the exact remainder, IS the correctly rounded quotient.  Three operations
// instead of the ~35 of a double division, once per (prefix, character) pair of every step.
__device__ __forceinline__ double div_ln10(float sc) {
  const double kLogE10 = 2.302585092994045684, kInv = 1.0 / 2.302585092994045684;
  const double x = (double)sc;
  const float a = fabsf(sc);
  if (a >= 0x1p-60f && a < 0x1p20f) {
    const double q0 = x * kInv;
    return fma(fma(-q0, kLogE10, x), kInv, q0);
  }
  return x / kLogE10;
}

// the LM part of get_next_prefix (:258-308) for the child (parent pr, char c), given the LM's answer for the pair
// (LM = false: the kernel instantiated for decoding without a language model touches num_words only -- the word
// insertion penalty needs it -- and none of the LM state, which otherwise costs the pair loop a third of its
// instructions and the kernel its scratch memory)
template <bool LM>
__device__ __forceinline__ void child_lm(const BeamParams& p, const LabelTab& lt, const LmFields& pr, int parent_last, int c, LmAnswer ans, LmFields& nn) {
  const bool new_word = c != p.space_id && (pr.num_words == 0 || parent_last == p.space_id);     // :258-259
  nn.num_words = pr.num_words + (new_word ? 1 : 0);
  nn.lm_score = 0.0; nn.num_oov = 0;
  if (!LM) return;
  nn.lm_before = 0.0; nn.num_oov_before = 0;
  nn.word_len = 0; nn.word_hash = kFnvInit; nn.st_n = 0; nn.stb_n = 0;
  if (c != p.space_id) {
    nn.word_hash = spell(p, lt, new_word ? kFnvInit : pr.word_hash, c);
    nn.word_len = (new_word ? 0 : pr.word_len) + 1;
    if (new_word) {                                                       // :265-281
      for (int s = 0; s < pr.st_n; s++) nn.stb[s] = pr.st[s];
      nn.stb_n = pr.st_n; nn.lm_before = pr.lm_score; nn.num_oov_before = pr.num_oov;
    } else {                                                              // :282-297
      for (int s = 0; s < pr.stb_n; s++) nn.stb[s] = pr.stb[s];
      nn.stb_n = pr.stb_n; nn.lm_before = pr.lm_before; nn.num_oov_before = pr.num_oov_before;
    }
    // the state after the word: the word, then the context it was scored in (lm_base_score's out_ctx)
    int m = nn.stb_n; if (m > p.lm.order - 1) m = p.lm.order - 1;
    m = m + 1; if (m > p.lm.order - 1) m = p.lm.order - 1;
    if (m > 0) nn.st[0] = ans.wi;
    for (int s = 1; s < m; s++) nn.st[s] = nn.stb[s - 1];
    nn.st_n = m;
    nn.lm_score = nn.lm_before + div_ln10(ans.sc);                 // quirk Q8: divides by ln 10
    nn.num_oov = nn.num_oov_before + (ans.wi == 0 ? 1 : 0);
  } else {                                                                // :299-307 copy
    nn.word_hash = pr.word_hash; nn.word_len = pr.word_len;
    nn.lm_score = pr.lm_score; nn.lm_before = pr.lm_before;
    nn.num_oov = pr.num_oov; nn.num_oov_before = pr.num_oov_before;
    for (int s = 0; s < pr.st_n; s++) nn.st[s] = pr.st[s];
    for (int s = 0; s < pr.stb_n; s++) nn.stb[s] = pr.stb[s];
    nn.st_n = pr.st_n; nn.stb_n = pr.stb_n;
  }
}
// ... and only what the score of the would-be prefix needs (the pair loop)
template <bool LM>
__device__ __forceinline__ void child_score_fields(const BeamParams& p, const LmFields& pr, int parent_last, int c, LmAnswer ans, LmFields& nn) {
  const bool new_word = c != p.space_id && (pr.num_words == 0 || parent_last == p.space_id);
  nn.num_words = pr.num_words + (new_word ? 1 : 0);
  nn.lm_score = 0.0; nn.num_oov = 0;
  if (!LM) return;
  if (c != p.space_id) {
    const double before = new_word ? pr.lm_score : pr.lm_before;
    const int oov_before = new_word ? pr.num_oov : pr.num_oov_before;
    nn.lm_score = before + div_ln10(ans.sc);
    nn.num_oov = oov_before + (ans.wi == 0 ? 1 : 0);
  } else {
    nn.lm_score = pr.lm_score; nn.num_oov = pr.num_oov;
  }
}

// get_prev_full_prob_with_lmwt, :314-318, from the already "next_step"-ed probabilities
template <bool LM>
__device__ __forceinline__ double beam_score_full(const BeamParams& p, double full, const LmFields& lm) {
  const double lm_score = LM ? lm.lm_score : 0.0;
  const int num_oov = LM ? lm.num_oov : 0;
  return full + lm_score * p.lmwt - lm.num_words * p.wip + num_oov * p.oov;
}
template <bool LM>
__device__ __forceinline__ double beam_score(const BeamParams& p, double ppnb, double ppb, const LmFields& lm) {
  // (without a language model lm_score and num_oov are zero for every prefix; the expression keeps its shape so that
  // the result has the reference's bits for any lmwt / oov the caller passes)
  const double lm_score = LM ? lm.lm_score : 0.0;
  const int num_oov = LM ? lm.num_oov : 0;
  return lse2(ppnb, ppb) + lm_score * p.lmwt - lm.num_words * p.wip + num_oov * p.oov;
}
template <bool LM>
__device__ __forceinline__ void copy_lm(LmFields& dst, const LmFields& src) {
  if (LM) dst = src; else dst.num_words = src.num_words;
}

// members of the beam, structure of arrays in LDS (two copies: the beam is rebuilt into the other one every step)
struct Members {
  double* ppb; double* ppnb;   // prev_prob_blank / prev_prob_not_blank
  double* npb; double* npnb;   // this step's prob_blank / prob_not_blank (become prev at next_step)
  double* inc;                 // contribution to prob_not_blank arriving from the parent (if it is in the beam)
  double* full;                // log_sum_exp(prev_pnb, prev_pb): carried from the previous step's score (nfull) / a new member's val
  double* nfull;               // log_sum_exp(npnb, npb), computed for this step's score
  int* node; int* last; int* kept;
  int* newpos;                 // position in the beam this step selects (valid where kept)
  int* gown; int* gchar; int* gnode;   // the member's guard (see the file header): owner's position (-1: none), character, node
  int* from;                   // position in the previous beam (-1: the member is new)
  LmFields* lm;
  __device__ unsigned char* carve(unsigned char* q, int W) {
    ppb = (double*)q; q += sizeof(double) * W; ppnb = (double*)q; q += sizeof(double) * W;
    npb = (double*)q; q += sizeof(double) * W; npnb = (double*)q; q += sizeof(double) * W;
    inc = (double*)q; q += sizeof(double) * W; full = (double*)q; q += sizeof(double) * W;
    nfull = (double*)q; q += sizeof(double) * W;
    lm = (LmFields*)q; q += sizeof(LmFields) * W;
    node = (int*)q; q += sizeof(int) * W; last = (int*)q; q += sizeof(int) * W;
    kept = (int*)q; q += sizeof(int) * W; newpos = (int*)q; q += sizeof(int) * W;
    gown = (int*)q; q += sizeof(int) * W; gchar = (int*)q; q += sizeof(int) * W;
    gnode = (int*)q; q += sizeof(int) * W;
    from = (int*)q; q += sizeof(int) * W;        // (an even number of int arrays: the next set starts 8-byte aligned)
    return q;
  }
  __host__ __device__ static size_t bytes(int W) { return (size_t)W * (7 * sizeof(double) + sizeof(LmFields) + 8 * sizeof(int)); }
};

struct BeamLds {
  static size_t bytes(int W, int V, int CMAX, int WP2, int HS, bool lm) {
    return sizeof(double) * ((size_t)CMAX + 2 * V + WP2 + kSelSmall) +
           sizeof(int) * ((size_t)WP2 + kSelSmall + 2 * (size_t)W * V + 2 * kSelBins + 64 + 4 * (size_t)HS) +
           2 * Members::bytes(W) + (lm ? 2 * sizeof(LmAnswer) * (size_t)W * V + sizeof(int) * (size_t)(2 * V + 2) + kLabelLdsBytes : 0) + 64;
  }
};

// Open addressing in LDS, int key -> int value, -1 an empty key.  SlotMap: node id -> position in the beam, for the <= W
// members, one table per member set (the table of the set that is being built is cleared a phase earlier); replaces a
// `slot` field in the HBM nodes that cost a global round trip per step to read.  ChildMap (the general kernel):
// (member position * V + character) -> node id of the alive child.
template <int kShift>
struct HashMap {
  int* key; int* val; int mask;
  __device__ static unsigned hash(int k) { return (unsigned)k * 2654435761u; }
  __device__ void insert(int k, int v) const {
    unsigned h = (hash(k) >> kShift) & mask;
    while (atomicCAS(&key[h], -1, k) != -1) h = (h + 1) & mask;
    val[h] = v;
  }
  __device__ int find(int k) const {
    unsigned h = (hash(k) >> kShift) & mask;
    for (;;) {
      const int kk = key[h];
      if (kk == k) return val[h];
      if (kk == -1) return -1;
      h = (h + 1) & mask;
    }
  }
};
typedef HashMap<8> SlotMap;
typedef HashMap<7> ChildMap;

// ---- the phases both kernels share ----
// The barrier a shared phase passes its data through: LDS only in the fast kernel, a full barrier in the general one (whose
// data crosses threads through global memory as well).
struct LdsSync { __device__ void operator()() const { lds_barrier(); } };
struct FullSync { __device__ void operator()() const { __syncthreads(); } };

// the root prefix (get_initial_prefix, :222-230) as member 0 of set 0 and node 0; one thread
__device__ __forceinline__ void init_root(const BeamParams& p, BeamNode* nodes, const Members& M0) {
  BeamNode& r = nodes[0];
  r.parent = -1; r.last_char = -1;
  LmFields l;
  l.lm_score = 0.0; l.lm_before = 0.0; l.num_words = 0; l.num_oov = 0; l.num_oov_before = 0; l.word_len = 0;
  l.word_hash = kFnvInit; l.st_n = 0; l.stb_n = 0;
  if (p.has_lm) { l.st[0] = p.lm.bos; l.st_n = 1; l.stb[0] = p.lm.bos; l.stb_n = 1; }
  M0.ppb[0] = 0.0; M0.ppnb[0] = ninf(); M0.full[0] = lse2(ninf(), 0.0); M0.inc[0] = ninf(); M0.kept[0] = 0; M0.node[0] = 0; M0.last[0] = -1; M0.gown[0] = -1; M0.gchar[0] = 0; M0.gnode[0] = 0;
  M0.lm[0] = l;
}

// ---- the phases of a streaming call (e2e_ctc_beam_stream), compiled into the kernels' ST instances only ----
// What the row says before a chunk of T frames: the frames consumed so far (fresh row: 0, resume = false) or a status < 0.
// The same for every thread of the workgroup (returned wave-uniform).
__device__ __forceinline__ int stream_open(const BeamParams& p, const unsigned char* row, int T, bool& resume) {
  const StreamHeader h = *reinterpret_cast<const StreamHeader*>(row);
  int st = 0, res = 0;
  if (h.magic != 0u) {
    const bool same = h.magic == kStreamMagic && h.V == p.V && h.W == p.W && h.has_lm == p.has_lm &&
                      h.max_frames == p.st_max_frames && h.with_ts == (p.st_ts_off ? 1 : 0) &&
                      h.n >= 1 && h.n <= p.W && h.next_node >= 1 && h.next_node <= p.NCAP && h.frames >= 0 && h.frames <= p.st_max_frames;
    if (same) { st = h.frames; res = 1; } else st = kStreamOtherConfig;
  }
  if (st >= 0 && st + T > p.st_max_frames) st = kStreamTooManyFrames;
  resume = __builtin_amdgcn_readfirstlane(res) != 0;
  return __builtin_amdgcn_readfirstlane(st);
}
// a status ends the utterance's workgroup before it touches anything: the row stays byte for byte what it was
__device__ __forceinline__ void stream_refuse(const BeamParams& p, int status) {
  if (threadIdx.x == 0) {
    p.frames_done[blockIdx.x] = status;
    if (p.nbest) p.n_hyp[blockIdx.x] = status;
  }
}
// resume: the stored member set becomes set 0 (all threads; the caller's barrier follows)
__device__ __forceinline__ void stream_load_members(unsigned char* set0, const unsigned char* row, size_t mbytes) {
  const unsigned long long* src = reinterpret_cast<const unsigned long long*>(row + kStreamHeaderBytes);
  unsigned long long* dst = reinterpret_cast<unsigned long long*>(set0);
  for (size_t i = threadIdx.x; i < mbytes / 8; i += kThreads) dst[i] = src[i];
}
// suspend, behind the chunk's last step: the current member set, then the header (plain vector stores).  A chunk of no frames
// stores nothing; neither does a chunk that ran out of nodes (err), whose status goes to frames_done.
__device__ __forceinline__ void stream_suspend(const BeamParams& p, unsigned char* row, const unsigned char* set, size_t mbytes,
                                               int n, int next_node, int t0, int T, int err) {
  if (!err && T > 0) {
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(set);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(row + kStreamHeaderBytes);
    for (size_t i = threadIdx.x; i < mbytes / 8; i += kThreads) dst[i] = src[i];
  }
  if (threadIdx.x == 0) {
    if (!err && T > 0) {
      StreamHeader h;
      h.magic = kStreamMagic; h.V = p.V; h.W = p.W; h.has_lm = p.has_lm; h.max_frames = p.st_max_frames; h.with_ts = p.st_ts_off ? 1 : 0;
      h.n = n; h.next_node = next_node; h.frames = t0 + T;
      *reinterpret_cast<StreamHeader*>(row) = h;
    }
    p.frames_done[blockIdx.x] = err ? kStreamPoolExhausted : t0 + T;
  }
}

// what the score of a member's would-be children needs of its LM state (only these fields are ever loaded)
template <bool LM>
__device__ __forceinline__ LmFields score_fields(const LmFields& m) {
  LmFields pr;
  pr.num_words = m.num_words;
  if (LM) { pr.lm_score = m.lm_score; pr.lm_before = m.lm_before; pr.num_oov = m.num_oov; pr.num_oov_before = m.num_oov_before; }
  return pr;
}
// the LM's answer for (member, character) at index i of an answer table (no language model: none)
template <bool LM, typename Idx>
__device__ __forceinline__ LmAnswer answer_at(const LmAnswer* lmc, Idx i) {
  LmAnswer ans; ans.sc = 0.f; ans.wi = 0u;
  if (LM) ans = lmc[i];
  return ans;
}
// the key of the would-be child (parent pr, char c) whose probability after next_step is prev_pnb = val, prev_pb = -inf
template <bool LM>
__device__ __forceinline__ unsigned long long child_key(const BeamParams& p, const LmFields& pr, int parent_last, int c, LmAnswer ans, double val) {
  LmFields nl;
  child_score_fields<LM>(p, pr, parent_last, c, ans, nl);
  return okey(beam_score<LM>(p, val, ninf(), nl));
}

// members: repeated-character share (:386-387), next_step (:337-342), score; row(c) is this step's log-probability of c.
// Each member's key goes to keys[i]; key_hi / key_lo collect the high words of the largest and of the smallest.
template <bool LM, class Row>
__device__ __forceinline__ void update_members(const BeamParams& p, const Members& A, int n, Row row, unsigned long long* keys,
                                               unsigned& key_hi, unsigned& key_lo) {
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const int lc = A.last[i];
    double pnb = A.inc[i];
    if (lc >= 0 && lc != p.blank) pnb = lse2(pnb, row(lc) + A.ppnb[i]);
    A.npnb[i] = pnb;
    const double nf = lse2(pnb, A.npb[i]);            // the score's log-sum-exp is next step's `full` if the member stays
    A.nfull[i] = nf;
    const double sc = beam_score_full<LM>(p, nf, A.lm[i]);
    const unsigned long long uk = okey(sc);
    keys[i] = uk;
    const unsigned h32 = (unsigned)(uk >> 32);
    key_hi = max(key_hi, h32); key_lo = min(key_lo, h32);
  }
}

// One digit of a radix select, once the digit's histogram hcur (kSelBins bins, the largest digit last) is complete: the digit
// where the running count from the top reaches krem.  Every thread owns kPer adjacent bins (one wave walking 32 bins per lane
// paid a 64-way bank conflict on every read) and zeroes them in hclear; found(rest, digit, count) is called by the one thread
// that owns the threshold digit (rest: how many of the digit's `count` keys are still wanted).  Leaves a Sync barrier behind
// the histogram reads and clears; the caller's barrier has to follow found().
template <class Sync, class Found>
__device__ __forceinline__ void select_digit(const int* hcur, int* hclear, int krem, int* s_part, Found found) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  constexpr int kPer = kSelBins / kThreads;
  static_assert(kPer * kThreads == kSelBins && kPer >= 1, "bins per thread");
  const int top = kSelBins - 1 - kPer * tid;
  int cnt[kPer], mine = 0;
#pragma unroll
  for (int jj = 0; jj < kPer; jj++) { cnt[jj] = hcur[top - jj]; mine += cnt[jj]; }
  const int inc = wave_scan_i(mine);
  if (lane == 63) s_part[wid] = inc;
#pragma unroll
  for (int jj = 0; jj < kPer; jj++) hclear[top - jj] = 0;
  Sync()();
  int above = inc - mine;                       // candidates with a larger digit than this thread's first
  {
    const int wtot = wave_scan_i(lane < kThreads / 64 ? s_part[lane] : 0);
    if (wid > 0) above += __builtin_amdgcn_readlane(wtot, wid - 1);
  }
  if (above < krem && above + mine >= krem) {   // the threshold digit is one of this thread's
#pragma unroll
    for (int jj = 0; jj < kPer; jj++) {
      if (above + cnt[jj] >= krem) { found(krem - above, top - jj, cnt[jj]); break; }
      above += cnt[jj];
    }
  }
}

// Rank of the M gathered candidates by (score desc, position asc): eight lanes count for one candidate.  emit(rank, e) for
// every candidate e whose rank -- its place in the new beam -- is below W.  kUnroll: comparisons in flight per lane (4 where
// emit is a store; where it builds the member, 4 would cost the general kernel two VGPRs spilled to scratch).
template <int kUnroll, class Emit>
__device__ __forceinline__ void rank_gathered(const unsigned long long* uskey, int M, int W, Emit emit) {
  const int tid = threadIdx.x;
  for (int e0 = 0; e0 < M; e0 += kThreads / 8) {
    const int e = e0 + (tid >> 3), part = tid & 7;
    int cnt = 0;
    if (e < M) {
      // (the gathered list is in position order within its two parts, and the keys of the first part are all
      // larger than those of the second: among equal keys the earlier list index is the earlier position)
      const unsigned long long ke = uskey[e];
#pragma unroll kUnroll
      for (int jj = part; jj < M; jj += 8) {
        const unsigned long long kj = uskey[jj];
        cnt += (kj > ke || (kj == ke && jj < e)) ? 1 : 0;
      }
    }
    cnt += __builtin_amdgcn_update_dpp(0, cnt, 0xB1, 0xf, 0xf, true);      // quad_perm [1,0,3,2]
    cnt += __builtin_amdgcn_update_dpp(0, cnt, 0x4E, 0xf, 0xf, true);      // quad_perm [2,3,0,1]
    cnt += __builtin_amdgcn_update_dpp(0, cnt, 0x141, 0xf, 0xf, true);     // row_half_mirror: the other quad of the 8
    if (e < M && part == 0 && cnt < W) emit(cnt, e);
  }
}

// ---- guards and child tables of the new beam Bm (nsel members) ----
// A guard whose owner left the beam is inherited from the owner's guard (the next alive prefix up the path whose
// parent was a member), until an owner that stays is found or the path runs out.  Every alive child of a member is
// some member's guard: writing the guards into the cleared tables -- store(member position * V + character, node) --
// reproduces exactly the entries whose weak_ptr has not expired upstream.
template <class Store>
__device__ __forceinline__ void rebuild_guards(const Members& A, const Members& Bm, int nsel, int V, Store store) {
  for (int j = threadIdx.x; j < nsel; j += kThreads) {
    Bm.inc[j] = ninf(); Bm.kept[j] = 0;                      // (what the next step's pair loop expects to find)
    int go = Bm.gown[j], gc = Bm.gchar[j], gn = Bm.gnode[j];
    while (go >= 0 && !A.kept[go]) { const int o = go; go = A.gown[o]; gc = A.gchar[o]; gn = A.gnode[o]; }
    if (go >= 0) {
      const int o = A.newpos[go];
      Bm.gown[j] = o; Bm.gchar[j] = gc; Bm.gnode[j] = gn;
      store(o * V + gc, gn);
    } else {
      Bm.gown[j] = -1;
    }
  }
}

// ---- final sort (:418-424) reduces to the best prefix; its sentence (:232-245) ----
// A: the n members after the last step; key: n doubles of scratch.  err: the node pool ran out.
template <bool LM>
__device__ __forceinline__ void read_out(const BeamParams& p, const Members& A, int n, double* key, const BeamNode* nodes,
                                         const int& err) {
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < n; i += kThreads) key[i] = beam_score<LM>(p, A.ppnb[i], A.ppb[i], A.lm[i]);
  __syncthreads();
  int64_t* out = p.out + (int64_t)b * p.max_out;
  for (int64_t i = tid; i < p.max_out; i += kThreads) out[i] = 0;
  __threadfence_block();
  __syncthreads();
  if (tid == 0) {
    int bi = 0;
    for (int i = 1; i < n; i++) if (key[i] > key[bi]) bi = i;            // first maximum = (score desc, position asc)
    const int best = A.node[bi];
    int64_t m = 0;
    for (int k = best; k >= 0; k = nodes[k].parent) if (k == best || nodes[k].parent >= 0) m++;
    int64_t at = m;
    for (int k = best; k >= 0; k = nodes[k].parent)
      if (k == best || nodes[k].parent >= 0) { at--; if (at < p.max_out) out[at] = nodes[k].last_char; }
    // in-band status (include/e2e_ctc.h): a length above max_out says "truncated, m were needed"; -1 = node pool
    // exhausted (the sentence is then that of the last completed step and must not be used)
    p.out_len[b] = err ? (int64_t)-1 : m;
  }
}

// ---- the n-best read-out: the final sort (:418-424) kept whole ----
// All n members of the last step are ranked by (score descending, position ascending) on the ordered key, as the search ranks
// its candidates; read_out()'s first maximum is rank 0.  The first N = min(nbest, n) get their sentence -- one lane per
// hypothesis, spread over the waves, so that the N chains of dependent loads run side by side and the tail of the call is one
// parent walk long, not N -- their scores and counts, and (node_t given) for every id the frame at which its node was created:
// a node is created exactly once and never reused, so this is the frame at which the label entered the beam on this path.
// ukey (n), order (n), lens (nbest): scratch in LDS that is dead after the last step.  Every element of every output row is
// written exactly once: by its walker up to the length, by the fill behind it.
template <bool LM>
__device__ __forceinline__ void read_out_nbest(const BeamParams& p, const Members& A, int n, unsigned long long* ukey, int* order,
                                               int* lens, const BeamNode* nodes, const int* node_t, const int& err) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = p.nbest, nh = n < N ? n : N;
  for (int i = tid; i < n; i += kThreads) ukey[i] = okey(beam_score<LM>(p, A.ppnb[i], A.ppb[i], A.lm[i]));
  __syncthreads();
  rank_gathered<4>(ukey, n, nh, [&](int rank, int e) { order[rank] = e; });
  __syncthreads();
  int64_t* const out = p.out + (int64_t)b * N * p.max_out;
  int64_t* const ts = p.ts_out ? p.ts_out + (int64_t)b * N * p.max_out : nullptr;
  int64_t* const out_len = p.out_len + (int64_t)b * N;
  double* const scores = p.scores + (int64_t)b * N * 3;
  int* const counts = p.counts + (int64_t)b * N * 2;
  const int every = kThreads / nh, h = tid / every;               // hypothesis h on thread h * every (nh <= W <= kThreads)
  if (h * every == tid && h < nh) {
    const int i = order[h], best = A.node[i];
    int m = 0;
    for (int k = best; k >= 0;) { const int par = nodes[k].parent; if (k == best || par >= 0) m++; k = par; }
    int64_t* const o = out + (int64_t)h * p.max_out;
    int64_t* const to = ts ? ts + (int64_t)h * p.max_out : nullptr;
    int at = m;
    for (int k = best; k >= 0;) {
      const BeamNode nd = nodes[k];
      if (k == best || nd.parent >= 0) {
        at--;
        if (at < p.max_out) {
          o[at] = nd.last_char;
          if (to) to[at] = nd.parent >= 0 ? node_t[k] : -1;        // (the root, an empty winner's -1, entered at no frame)
        }
      }
      k = nd.parent;
    }
    lens[h] = m;
    out_len[h] = m;                                                // (in-band status as in read_out: > max_out = truncated)
    const double ctc = lse2(A.ppnb[i], A.ppb[i]);
    scores[3 * h] = beam_score<LM>(p, A.ppnb[i], A.ppb[i], A.lm[i]);
    scores[3 * h + 1] = ctc;
    scores[3 * h + 2] = LM ? A.lm[i].lm_score : 0.0;
    counts[2 * h] = A.lm[i].num_words;
    counts[2 * h + 1] = LM ? A.lm[i].num_oov : 0;
  }
  for (int e = nh + tid; e < N; e += kThreads) {                   // fewer members than asked for
    out_len[e] = 0; lens[e] = 0;
    scores[3 * e] = ninf(); scores[3 * e + 1] = ninf(); scores[3 * e + 2] = 0.0;
    counts[2 * e] = 0; counts[2 * e + 1] = 0;
  }
  if (tid == 0) p.n_hyp[b] = err ? (int64_t)-1 : (int64_t)nh;      // -1: node pool exhausted, nothing of this utterance may be used
  __syncthreads();
  for (int e = 0; e < N; e++) {
    const int64_t from = lens[e] < p.max_out ? lens[e] : p.max_out;
    for (int64_t i = from + tid; i < p.max_out; i += kThreads) { out[e * p.max_out + i] = 0; if (ts) ts[e * p.max_out + i] = -1; }
  }
}

// ---- what the host fills in for the general kernel (ctc_beam_general.hip has the kernel and the account of it) ----
constexpr int kGenMaxW = 1024;

// Character pre-selection of the general kernel (no language model): capacity of the per-step character list and words of
// the character bitmap in LDS (alphabets beyond 2^16 columns take every character, as before).
__host__ __device__ inline int gen_list_cap(int W) { return 4 * W + 64; }
__host__ __device__ inline int gen_bitmap_words(int V) { return V <= 65536 ? (V + 31) / 32 : 1; }
struct GenParams {
  unsigned long long* gkey;      // [B][gstride]
  LmAnswer* lmc;                 // [B][2][W][V]   (null without a language model, and in a pruned call)
  unsigned char* gmem;           // [B][2][Members::bytes(W)]: both member sets, when they no longer fit LDS (else null)
  int CH;                        // child map slots (power of two >= 4W)
  // A pruned call (e2e_ctc_beam_nbest_cut, the kernel's CUT instances): the frames' label lists, written by the selection
  // kernel ahead of this one on the stream.  Every other call reads nothing below.
  const int* cut_ids;            // [B][T][cut_k1] ascending, -1 behind
  const int* cut_n;              // [B][T]
  int cut_k1;                    // min(cutoff_top_n, V) + 1
  size_t gstride;                // candidate keys of an utterance: W + W * V, pruned W + W * cut_k1
};

// ---- per-frame label pruning (ctc_label_cut.hip): what the pruned search's host side needs of it ----
inline int label_cut_k(int V, int cutoff_top_n) { return cutoff_top_n < V ? cutoff_top_n : V; }
// the argument errors of a selection (E2E_ERR_ARG, the limit: E2E_ERR_UNSUPPORTED), before any launch
int label_cut_check(int dtype, int B, int T, int V, int blank, int cutoff_top_n, double cutoff_prob);
// blank < 0: no blank (asg_beam_cut.hip; f32 / f64, V <= 256, cutoff_prob 1): ids is (B,T,K), a frame's count is K
int launch_label_cut(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len, int B, int T, int V,
                     int blank, int cutoff_top_n, double cutoff_prob, int* ids, int* n, hipStream_t s);

// ---- the kernel objects ----
// Instance <IO, lmk, st> of a kernel, for its launch.  Each specialisation is defined by the object of its dtype; an lmk
// outside [0, kLmKinds) is the caller's error (lmk_of gives none).
template <typename IO> const void* lds_kernel(int lmk, bool st);
template <typename IO, bool CUT> const void* general_kernel(int lmk, bool st);     // (CUT: the pruned calls' instances)
template <> const void* lds_kernel<float>(int, bool);
template <> const void* lds_kernel<double>(int, bool);
template <> const void* lds_kernel<f16_t>(int, bool);
template <> const void* lds_kernel<bf16_t>(int, bool);
template <> const void* general_kernel<float, false>(int, bool);
template <> const void* general_kernel<double, false>(int, bool);
template <> const void* general_kernel<f16_t, false>(int, bool);
template <> const void* general_kernel<bf16_t, false>(int, bool);
template <> const void* general_kernel<float, true>(int, bool);
template <> const void* general_kernel<double, true>(int, bool);
template <> const void* general_kernel<f16_t, true>(int, bool);
template <> const void* general_kernel<bf16_t, true>(int, bool);

}  // namespace beamk
}  // namespace e2e
