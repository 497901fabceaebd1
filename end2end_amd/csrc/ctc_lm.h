// The n-gram language model: table layout and lookups shared by the host scorer and the beam kernels (ctc_beam.hip),
// and the host-side model (struct e2e_lm) that ctc_lm.hip loads and e2e_ctc_beam reads.
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"

namespace e2e {

constexpr int kLmMaxOrder = 6;     // KENLM_MAX_ORDER=6, CMakeLists.txt:36
constexpr int kCtx = kLmMaxOrder - 1;

struct NgSlot { uint32_t ids[kLmMaxOrder]; int32_t n; float prob; float backoff; };
// The same tables in the form the kernel probes: one 16-byte load per probe, matched by the n-gram's 64-bit hash
// (the loader checks that no two n-grams of the model share one; a queried n-gram that is NOT in the model would have
// to collide in all 64 bits with the entry at its probe position to be mistaken for it).
struct NgSig {                                                   // sig 0: empty
  uint64_t sig; float prob; float backoff;
  // second half, read for CONTEXT lookups only: one bit per continuation word of this n-gram (bit cont_bit(w) is set if the
  // model lists (this n-gram, w)).  A query's longer n-grams are only looked up when their context says they may exist:
  // what a beam step asks is bound by the number of distinct cache lines its waves touch, and for most
  // (context, word) pairs a beam search tries there is no such n-gram.  No false negatives; contexts with many
  // continuations fill their 64 bits and every lookup is made, as before.
  uint64_t cont; uint64_t pad;
};
// Unigrams are not hashed at all: one 16-byte entry per word id (prob > 0: the model has no such unigram).  A few hundred
// KB that stay in L2, where the hashed table (megabytes, one slot per random line) is a trip past it for every probe.
struct UniEntry { float prob; float backoff; uint64_t cont; };
__host__ __device__ inline int cont_bit(uint32_t w) { return (int)(((uint64_t)w * 0x9E3779B97F4A7C15ULL) >> 58); }
struct VEntry { uint64_t key; uint32_t val; float prob; };       // key 0: empty; prob: the word's unigram log10 p (> 0: none listed)
// The kernel's vocabulary table is a TWO-CHOICE (cuckoo) table: a spelling sits in one of the two slots its hash names, so a
// probe is two loads issued together and never a second round (with linear probing the slowest of a wave's 64 lanes needed
// three).  It is small -- 64 bytes per word -- and stays in L2, where a second line per probe is cheap.  (The n-gram table
// keeps linear probing: since the continuation bits its probes are rare or shared by a state's characters.)
__host__ __device__ inline void two_slots(uint64_t h, uint32_t mask, uint32_t& i1, uint32_t& i2) {
  // (the second slot from a re-mixed hash: bits 32.. of an FNV hash of a short spelling are far from uniform -- 7 191
  //  distinct values for the bench model's 10 003 words -- and cuckoo insertion then fails)
  i1 = (uint32_t)h & mask; i2 = (uint32_t)((h * 0x9E3779B97F4A7C15ULL) >> 32) & mask;
  if (i2 == i1) i2 = i1 ^ 1u;
}

struct LmView {                    // what the kernel sees (device pointers) / what the host scorer sees
  int order;
  const uint64_t* vkeys; const uint32_t* vvals; uint32_t vmask;
  const NgSlot* ng; uint32_t ngmask;
  uint32_t bos;
  const unsigned char* label_bytes; const int* label_off;   // label c spells bytes [off[c], off[c+1])
  int fold_case;
  const NgSig* ngs; const VEntry* vt;                        // device only (null: n-gram hashes collide, use ng / vkeys)
  const UniEntry* uni; uint32_t nwords;                      // device only, with ngs
  float unk_prob;                                            // p(<unk>) (KenLM's -100 if the model has none)
  const uint32_t* homs;                                      // transcription models: the homophone sets (count, ids ...); else null
};

// Custom transcriptions (e2e_lm_load_transcriptions): the vocabulary tables are keyed by a word's sequence of label ids
// -- label c spells the two bytes of c + 1, so the kernel's spell() hashes ids, not characters -- and one key may belong
// to several words (homophones).  A key with one word stores its id as always; a key with several stores kHomMark | offset
// into LmView::homs, where the set lies as (count, id_1 .. id_count) in the order of the lexicon.  Only the language model
// can choose between homophones: the word of such a key is the one with the greatest score in the asking prefix's context,
// exact ties to the earliest listed (lm_query in ctc_beam.hip, e2e_lm_transcribe on the host).
constexpr uint32_t kHomMark = 0x80000000u;
constexpr int kMaxHomophones = 16;
constexpr int kMaxTranscription = 255;
__host__ __device__ inline bool is_hom_ref(uint32_t val) { return (val & kHomMark) != 0; }   // (a table value; never kNoChildWord)

__host__ __device__ inline uint64_t fnv_step(uint64_t h, unsigned char b) { return (h ^ b) * 1099511628211ULL; }
constexpr uint64_t kFnvInit = 1469598103934665603ULL;
// the hash h of a spelling, extended by label c's bytes (the searches that spell from the model's own strings: asg_beam.hip,
// ctc_gram_decode.hip)
__device__ __forceinline__ unsigned long long spell(const LmView& lm, unsigned long long h, int c) {
  for (int bi = lm.label_off[c]; bi < lm.label_off[c + 1]; bi++) {
    unsigned char ch = lm.label_bytes[bi];
    if (lm.fold_case && ch >= 'A' && ch <= 'Z') ch += 32;
    h = fnv_step(h, ch);
  }
  return h;
}

// hash of an n-gram of word ids (table placement and signature; internal to the LM code): one multiply per id
__host__ __device__ inline uint64_t ng_mix(uint64_t h, uint32_t id) { h = (h ^ id) * 0x9E3779B97F4A7C15ULL; return h ^ (h >> 32); }
__host__ __device__ inline uint64_t ng_finish(uint64_t h, int n) { h = ng_mix(h, 0x51ED2700u + (uint32_t)n); return h == 0 ? 1 : h; }
__host__ __device__ inline uint64_t ngram_hash(const uint32_t* ids, int n) {
  uint64_t h = kFnvInit;
  for (int i = 0; i < n; i++) h = ng_mix(h, ids[i]);
  return ng_finish(h, n);
}

__host__ __device__ inline uint32_t lm_word_lookup(const LmView& lm, uint64_t h) {
  if (h == 0) h = 1;
  for (uint32_t i = (uint32_t)h & lm.vmask;; i = (i + 1) & lm.vmask) {
    const uint64_t k = lm.vkeys[i];
    if (k == h) return lm.vvals[i];
    if (k == 0) return 0;                       // NotFound() == <unk> == 0
  }
}

// ... and whether the spelling is in the table at all.  A model with a lexicon (e2e_lm_enable_lexicon) also lists every proper
// prefix of a word that is no word itself, with id 0: to an unrestricted lookup such an entry is the miss it always was, to a
// search restricted to the lexicon it says "this spelling may go on".
__host__ __device__ inline bool lm_word_find(const LmView& lm, uint64_t h, uint32_t& id) {
  if (h == 0) h = 1;
  for (uint32_t i = (uint32_t)h & lm.vmask;; i = (i + 1) & lm.vmask) {
    const uint64_t k = lm.vkeys[i];
    if (k == h) { id = lm.vvals[i]; return true; }
    if (k == 0) { id = 0; return false; }
  }
}

__host__ __device__ inline const NgSlot* lm_ngram_find(const LmView& lm, const uint32_t* ids, int n) {
  for (uint32_t i = (uint32_t)ngram_hash(ids, n) & lm.ngmask;; i = (i + 1) & lm.ngmask) {
    const NgSlot* s = &lm.ng[i];
    if (s->n == 0) return nullptr;
    if (s->n == n) {
      bool eq = true;
      for (int k = 0; k < n; k++) eq = eq && s->ids[k] == ids[k];
      if (eq) return s;
    }
  }
}

// log10 p(word | ctx) with ARPA back-off; ctx is most-recent-first.  Float accumulation in KenLM's order: the prob of
// the longest listed n-gram, then the back-off weights of the longer contexts, shortest context first.
__host__ __device__ inline float lm_base_score(const LmView& lm, const uint32_t* ctx, int ctx_len, uint32_t word,
                                               uint32_t* out_ctx, int* out_len) {
  int n = ctx_len; if (n > lm.order - 1) n = lm.order - 1;
  uint32_t ids[kLmMaxOrder];
  float bo[kLmMaxOrder + 1];
  float result = 0.f; int found_k = -1;
  for (int k = n; k >= 0; k--) {
    for (int i = 0; i < k; i++) ids[i] = ctx[k - 1 - i];
    ids[k] = word;
    const NgSlot* s = lm_ngram_find(lm, ids, k + 1);
    if (s) { result = s->prob; found_k = k; break; }
    bo[k] = 0.f;
    if (k > 0) { const NgSlot* c = lm_ngram_find(lm, ids, k); if (c) bo[k] = c->backoff; }
  }
  if (found_k < 0) { const uint32_t z = 0; const NgSlot* u = lm_ngram_find(lm, &z, 1); result = u ? u->prob : -100.f; found_k = 0; }
  for (int k = found_k + 1; k <= n; k++) result += bo[k];
  if (out_ctx) {
    int m = n + 1; if (m > lm.order - 1) m = lm.order - 1;
    uint32_t tmp[kLmMaxOrder];
    if (m > 0) tmp[0] = word;
    for (int i = 1; i < m; i++) tmp[i] = ctx[i - 1];
    for (int i = 0; i < m; i++) out_ctx[i] = tmp[i];
    *out_len = m;
  }
  return result;
}

// the word of a homophone set in the context ctx: greatest lm_base_score, exact ties to the earliest listed
__host__ __device__ inline uint32_t lm_homophone_choice(const LmView& lm, uint32_t ref, const uint32_t* ctx, int ctx_len, float* score) {
  const uint32_t* set = lm.homs + (ref & ~kHomMark);
  const uint32_t count = set[0];
  uint32_t best = set[1];
  float best_sc = lm_base_score(lm, ctx, ctx_len, best, nullptr, nullptr);
  for (uint32_t i = 1; i < count; i++) {
    const float sc = lm_base_score(lm, ctx, ctx_len, set[1 + i], nullptr, nullptr);
    if (sc > best_sc) { best_sc = sc; best = set[1 + i]; }
  }
  *score = best_sc;
  return best;
}

}  // namespace e2e

// ------------------------------------------------------------------------------------------------------
// host side of the LM
// ------------------------------------------------------------------------------------------------------
struct e2e_lm {
  int order = 0;
  int fold_case = 0;
  std::vector<uint64_t> vkeys; std::vector<uint32_t> vvals;
  std::vector<e2e::NgSlot> ng;
  std::vector<unsigned char> label_bytes; std::vector<int> label_off;
  std::unordered_map<std::string, uint32_t> exact;       // word -> id, exact case (GetVocabulary().Index)
  uint32_t bos = 0;
  // device copies
  uint64_t* d_vkeys = nullptr; uint32_t* d_vvals = nullptr; e2e::NgSlot* d_ng = nullptr;
  unsigned char* d_label_bytes = nullptr; int* d_label_off = nullptr;
  e2e::NgSig* d_ngs = nullptr; e2e::VEntry* d_vt = nullptr;     // (d_ngs stays null if two n-grams share a hash)
  e2e::UniEntry* d_uni = nullptr; uint32_t nwords = 0;
  float unk_prob = -100.f;
  // the lexicon (e2e_lm_enable_lexicon): folded spelling -> bit 0 a word, bit 1 a proper prefix of a longer word.  Once it is
  // built, the vocabulary tables above also hold the prefixes that are no words, with id 0.
  bool has_lexicon = false;
  bool words_only = false;                               // e2e_lm_load_words: the model that scores nothing
  std::unordered_map<std::string, unsigned char> lex_class;
  int device = -1;                                       // HIP device that holds the tables (-1: host only)
  std::vector<std::string> words;                        // id -> word as the model lists it (e2e_lm_word_string)
  // custom transcriptions (e2e_lm_load_transcriptions): fold_case still folds the WORDS; the label bytes are id codes and
  // are never folded.  `folded`: folded word -> id, what the vocabulary table says of a model that spells its words.
  bool transcribed = false;
  int transcriptions_dropped = 0;
  std::vector<uint32_t> homs; uint32_t* d_homs = nullptr;
  std::unordered_map<std::string, uint32_t> folded;
  std::vector<std::string> tr_keys;                      // the kept transcriptions, as id codes (the lexicon of such a model)
  e2e::LmView host_view() const {
    return {order, vkeys.data(), vvals.data(), (uint32_t)vkeys.size() - 1, ng.data(), (uint32_t)ng.size() - 1, bos,
            label_bytes.data(), label_off.data(), transcribed ? 0 : fold_case, nullptr, nullptr, nullptr, nwords, unk_prob,
            homs.data()};
  }
  e2e::LmView dev_view() const {
    return {order, d_vkeys, d_vvals, (uint32_t)vkeys.size() - 1, d_ng, (uint32_t)ng.size() - 1, bos,
            d_label_bytes, d_label_off, transcribed ? 0 : fold_case, d_ngs, d_ngs ? d_vt : nullptr, d_ngs ? d_uni : nullptr,
            nwords, unk_prob, d_homs};
  }
};

namespace e2e {
// E2E_OK if a call on the current device may read the model's tables (lm null: no model, nothing to read), else the error
// set: no device tables, or tables on another device (ctc_lm.hip)
int check_model_device(const e2e_lm* lm);
// The argument errors the three beam searches (ctc_beam.hip, asg_beam.hip, ctc_gram_decode.hip) word alike: E2E_OK, else the
// error set.  A search restricted to the lexicon has a model, and one with a lexicon ...
int check_lexicon(const e2e_lm* lm, bool restricted);
// ... a stream's state rows are at least `want` bytes -- what the entry's own query, named `query`, says -- and a multiple of 8 ...
int check_row_bytes(size_t row_bytes, size_t want, const char* query);
// ... and the state is 8-byte aligned (not looked at for B = 0)
int check_state_aligned(int B, const void* state);
}  // namespace e2e
