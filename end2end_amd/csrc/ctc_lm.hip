// The n-gram language model on the host: ARPA reader (plain or gzip), the device tables' upload and their self-check, and
// the e2e_lm_* exports.  Restates KenLM's part upstream (src/decoders/ctc_decoder.cpp:60-71,77-88).
#include <zlib.h>

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include <stdlib.h>

#include "ctc_lm.h"

namespace e2e {
namespace {

uint64_t word_hash(const std::string& w) {
  uint64_t h = kFnvInit;
  for (unsigned char c : w) h = fnv_step(h, c);
  return h == 0 ? 1 : h;
}

size_t pow2_at_least(size_t n) { size_t p = 16; while (p < n) p <<= 1; return p; }

std::string lower(const std::string& s) {
  std::string r = s;
  for (auto& c : r) c = (char)::tolower((unsigned char)c);      // str_to_lower, ctc_decoder.cpp:32-36
  return r;
}

struct Entry { uint32_t ids[kLmMaxOrder]; int n; float prob, bo; };

// cuckoo insertion into the kernel's two-choice vocabulary table: a free slot of the item's two, else evict the occupant of
// one and move that on
bool cuckoo_insert(std::vector<VEntry>& vt, VEntry item) {
  const uint32_t mask = (uint32_t)vt.size() - 1;
  uint32_t i1, i2;
  two_slots(item.key, mask, i1, i2);
  if (vt[i1].key == 0) { vt[i1] = item; return true; }
  if (vt[i2].key == 0) { vt[i2] = item; return true; }
  uint32_t pos = i1;
  for (int kick = 0; kick < 2000; kick++) {
    std::swap(item, vt[pos]);
    if (item.key == 0) return true;
    two_slots(item.key, mask, i1, i2);
    pos = pos == i1 ? i2 : i1;
  }
  return false;
}

bool upload(void** d, const void* h, size_t bytes) {
  if (hipMalloc(d, bytes) != hipSuccess) return false;
  return hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice) == hipSuccess;
}

bool is_special(const std::string& w) { return w == "<unk>" || w == "<s>" || w == "</s>"; }

}  // namespace
}  // namespace e2e

using namespace e2e;

// a transcription key: the id code of its labels (two bytes per label), its hash, and its words in the lexicon's order
struct TrKey { std::string code; uint64_t h; std::vector<uint32_t> ids; };

static void build_model(e2e_lm* lm, const std::vector<std::string>& words, std::vector<Entry>& entries,
                        const char* const* labels, int V, const std::vector<TrKey>* keys = nullptr);

// reads an ARPA file into a fresh model: its words (lm->exact, id -> word) and n-grams; the tables are build_model's
static int read_arpa(const char* path, int case_sensitive, e2e_lm** out, std::vector<std::string>& words, std::vector<Entry>& entries) {
  gzFile f = gzopen(path, "rb");
  if (!f) { set_error("cannot open language model %s", path); return E2E_ERR_IO; }
  {
    // KenLM's own binary format (what `build_binary` writes; upstream's LoadVirtual, ctc_decoder.cpp:64, takes it too)
    // is not read here: say so instead of failing to find ARPA sections
    char magic[64] = {0};
    const int got = gzread(f, magic, sizeof(magic) - 1);
    if (got > 0 && strncmp(magic, "mmap lm http://kheafield.com/code", 33) == 0) {
      gzclose(f);
      set_error("%s is a KenLM binary model; this library reads ARPA (plain or .gz) -- convert it back with KenLM, or "
                "load the ARPA file it was built from", path);
      return E2E_ERR_UNSUPPORTED;
    }
    gzrewind(f);
  }
  e2e_lm* lm = new e2e_lm();
  lm->fold_case = case_sensitive ? 0 : 1;
  auto intern = [&](const std::string& w) -> uint32_t {
    auto it = lm->exact.find(w);
    if (it != lm->exact.end()) return it->second;
    const uint32_t id = (uint32_t)words.size();
    words.push_back(w); lm->exact.emplace(w, id);
    return id;
  };
  intern("<unk>");                                         // id 0 is <unk>
  std::vector<char> buf(1 << 16);
  int section = 0; bool saw_data = false;
  while (gzgets(f, buf.data(), (int)buf.size())) {
    char* line = buf.data();
    size_t len = strlen(line);
    while (len > 0 && (line[len - 1] == '\n' || line[len - 1] == '\r')) line[--len] = 0;
    if (len == 0) continue;
    if (line[0] == '\\') {
      int k;
      if (strncmp(line, "\\data\\", 6) == 0) saw_data = true;
      else if (sscanf(line, "\\%d-grams:", &k) == 1) { section = k; if (k > lm->order) lm->order = k; }
      else if (strncmp(line, "\\end\\", 5) == 0) break;
      continue;
    }
    if (section == 0 || section > kLmMaxOrder) continue;
    char* save = nullptr;
    char* tok = strtok_r(line, " \t", &save);
    if (!tok) continue;
    Entry e; e.n = section; e.prob = strtof(tok, nullptr); e.bo = 0.f;
    bool ok = true;
    for (int i = 0; i < section; i++) { tok = strtok_r(nullptr, " \t", &save); if (!tok) { ok = false; break; } e.ids[i] = intern(tok); }
    if (!ok) continue;
    tok = strtok_r(nullptr, " \t", &save);
    if (tok) e.bo = strtof(tok, nullptr);
    entries.push_back(e);
  }
  gzclose(f);
  if (!saw_data || lm->order == 0) { delete lm; set_error("%s: not an ARPA file (no \\data\\ / n-gram sections)", path); return E2E_ERR_IO; }
  if (lm->order > kLmMaxOrder) { delete lm; set_error("%s: order %d > %d", path, lm->order, kLmMaxOrder); return E2E_ERR_UNSUPPORTED; }
  *out = lm;
  return E2E_OK;
}

extern "C" int e2e_lm_load_arpa(const char* path, const char* const* labels, int V, int case_sensitive, e2e_lm** out) {
  if (out) *out = nullptr;
  if (!path || !out || V < 0 || (V > 0 && !labels)) { set_error("e2e_lm_load_arpa: bad argument"); return E2E_ERR_ARG; }
  std::vector<std::string> words;
  std::vector<Entry> entries;
  e2e_lm* lm = nullptr;
  const int rc = read_arpa(path, case_sensitive, &lm, words, entries);
  if (rc != E2E_OK) return rc;
  build_model(lm, words, entries, labels, V);
  *out = lm;
  return E2E_OK;
}

// The tables of a model whose words (id -> word, lm->exact filled) and n-grams have been read: the id-keyed host tables, the
// kernel's forms of them, their self-check and their upload to the current device.  With `keys` (custom transcriptions) the
// vocabulary tables are keyed by those instead of the words' spellings, and label c spells the two bytes of c + 1.
static void build_model(e2e_lm* lm, const std::vector<std::string>& words, std::vector<Entry>& entries,
                        const char* const* labels, int V, const std::vector<TrKey>* keys) {
  lm->words = words;
  {  // <unk> absent from the file: KenLM's default unknown_missing_logprob = -100
    bool has_unk = false;
    for (const auto& e : entries) if (e.n == 1 && e.ids[0] == 0) { has_unk = true; break; }
    if (!has_unk) { Entry e; e.n = 1; e.ids[0] = 0; e.prob = -100.f; e.bo = 0.f; entries.push_back(e); }
  }
  // n-gram table
  // (load <= 1/4: most misses end at the first slot.  The table's footprint is not what the kernel's queries cost: 2, 3, 4, 8
  //  slots per entry -- 2 to 8 MB for the bench's model -- measured 28.0 / 26.6 / 26.6 / 26.1 ms per C4 batch.)
  lm->ng.assign(pow2_at_least(entries.size() * 4 + 16), NgSlot{{0, 0, 0, 0, 0, 0}, 0, 0.f, 0.f});
  const uint32_t ngmask = (uint32_t)lm->ng.size() - 1;
  for (const auto& e : entries) {
    uint32_t i = (uint32_t)ngram_hash(e.ids, e.n) & ngmask;
    for (;; i = (i + 1) & ngmask) {
      NgSlot& s = lm->ng[i];
      if (s.n == 0) { s.n = e.n; for (int k = 0; k < e.n; k++) s.ids[k] = e.ids[k]; s.prob = e.prob; s.backoff = e.bo; break; }
      if (s.n == e.n && memcmp(s.ids, e.ids, sizeof(uint32_t) * e.n) == 0) { s.prob = e.prob; s.backoff = e.bo; break; }
    }
  }
  // vocabulary table keyed by the hash of the (optionally lower-cased) spelling; when two words fold to the same
  // string the reference keeps whichever its unordered_map iteration visits last (unspecified) -- here: lowest id
  lm->vkeys.assign(pow2_at_least((keys ? keys->size() : words.size()) * 4 + 16), 0);
  lm->vvals.assign(lm->vkeys.size(), 0);
  const uint32_t vmask = (uint32_t)lm->vkeys.size() - 1;
  auto vput = [&](uint64_t h, uint32_t val) {
    for (uint32_t i = (uint32_t)h & vmask;; i = (i + 1) & vmask) {
      if (lm->vkeys[i] == h) break;
      if (lm->vkeys[i] == 0) { lm->vkeys[i] = h; lm->vvals[i] = val; break; }
    }
  };
  if (!keys) {
    for (uint32_t id = 0; id < words.size(); id++) vput(word_hash(lm->fold_case ? lower(words[id]) : words[id]), id);
  } else {
    lm->transcribed = true;
    for (const TrKey& k : *keys) {
      if (k.ids.size() == 1) { vput(k.h, k.ids[0]); continue; }
      vput(k.h, kHomMark | (uint32_t)lm->homs.size());
      lm->homs.push_back((uint32_t)k.ids.size());
      lm->homs.insert(lm->homs.end(), k.ids.begin(), k.ids.end());
    }
    if (lm->homs.empty()) lm->homs.push_back(0);
  }
  { auto it = lm->exact.find("<s>"); lm->bos = it != lm->exact.end() ? it->second : 0; }
  lm->label_off.assign(1, 0);
  for (int c = 0; c < V; c++) {
    if (keys) { lm->label_bytes.push_back((unsigned char)((c + 1) & 255)); lm->label_bytes.push_back((unsigned char)((c + 1) >> 8)); }
    else for (const char* s = labels[c]; *s; s++) lm->label_bytes.push_back((unsigned char)*s);
    lm->label_off.push_back((int)lm->label_bytes.size());
  }
  if (lm->label_bytes.empty()) lm->label_bytes.push_back(0);
  auto up = upload;
  // the kernel's 16-byte forms of the two tables (same slots)
  std::vector<NgSig> ngs(lm->ng.size(), NgSig{0, 0.f, 0.f, 0, 0});
  std::vector<UniEntry> uni(words.size(), UniEntry{1.f, 0.f, 0});
  lm->nwords = (uint32_t)words.size();
  bool sig_ok = true;
  {
    std::vector<uint64_t> seen;
    seen.reserve(entries.size());
    for (size_t i = 0; i < lm->ng.size(); i++) {
      const NgSlot& sl = lm->ng[i];
      if (sl.n == 0) continue;
      ngs[i].sig = ngram_hash(sl.ids, sl.n); ngs[i].prob = sl.prob; ngs[i].backoff = sl.backoff;
      seen.push_back(ngs[i].sig);
      if (sl.n == 1 && sl.ids[0] == 0) lm->unk_prob = sl.prob;
    }
    std::sort(seen.begin(), seen.end());
    sig_ok = std::adjacent_find(seen.begin(), seen.end()) == seen.end();
    // continuation bits: (w1 .. wn) sets bit cont_bit(wn) of its context (w1 .. wn-1).  The kernel's scorer
    // (lm_score_parallel) looks an n-gram up only behind a HIT of its context, so a model that lists an n-gram without its
    // context (SRILM-pruned files do; KenLM inserts blank entries for them) cannot use these tables: the id-keyed walk
    // (lm_base_score), which probes every order, takes over.
    bool contexts_listed = true;
    const LmView hv = lm->host_view();
    for (size_t i = 0; i < lm->ng.size(); i++) {
      const NgSlot& sl = lm->ng[i];
      if (sl.n == 1) { uni[sl.ids[0]].prob = sl.prob; uni[sl.ids[0]].backoff = sl.backoff; }
    }
    for (size_t i = 0; i < lm->ng.size() && contexts_listed; i++) {
      const NgSlot& sl = lm->ng[i];
      if (sl.n < 2) continue;
      const NgSlot* c = lm_ngram_find(hv, sl.ids, sl.n - 1);
      if (!c) { contexts_listed = false; break; }
      const uint64_t bit = 1ULL << cont_bit(sl.ids[sl.n - 1]);
      if (sl.n == 2) uni[sl.ids[0]].cont |= bit; else ngs[(size_t)(c - lm->ng.data())].cont |= bit;
    }
    if (!contexts_listed) {
      sig_ok = false;
      if (getenv("E2E_LM_DEBUG")) fprintf(stderr, "e2e_lm: an n-gram's context is not listed; using the id tables (slower)\n");
    }
  }
  std::vector<VEntry> vt(lm->vkeys.size(), VEntry{0, 0u, 1.f});
  for (size_t i = 0; i < lm->vkeys.size() && sig_ok; i++) {      // (one entry per distinct folded spelling already)
    if (lm->vkeys[i] == 0) continue;
    if (!cuckoo_insert(vt, VEntry{lm->vkeys[i], lm->vvals[i], is_hom_ref(lm->vvals[i]) ? 1.f : uni[lm->vvals[i]].prob}))
      sig_ok = false;                                               // (never seen at load <= 1/4; the id-keyed walk takes over)
  }
  // Self-check of what the kernel will read, against the id tables it stands for: every spelling is found in one of its two
  // vocabulary slots with the right id and unigram; every listed n-gram is found by its signature with the right numbers and
  // its context lists its last word.  (What is NOT listed can only cost a wasted lookup: the filters have no false negatives.)
  if (sig_ok) {
    const uint32_t vmask2 = (uint32_t)vt.size() - 1;
    for (size_t i = 0; i < lm->vkeys.size() && sig_ok; i++) {
      if (lm->vkeys[i] == 0) continue;
      uint32_t i1, i2;
      two_slots(lm->vkeys[i], vmask2, i1, i2);
      const VEntry* e = vt[i1].key == lm->vkeys[i] ? &vt[i1] : vt[i2].key == lm->vkeys[i] ? &vt[i2] : nullptr;
      sig_ok = e && e->val == lm->vvals[i] && (is_hom_ref(e->val) || e->prob == uni[e->val].prob);
    }
    const LmView hv = lm->host_view();
    for (size_t i = 0; i < lm->ng.size() && sig_ok; i++) {
      const NgSlot& sl = lm->ng[i];
      if (sl.n == 0) continue;
      const uint64_t sig = ngram_hash(sl.ids, sl.n);
      uint32_t j = (uint32_t)sig & ngmask;
      while (ngs[j].sig != sig && ngs[j].sig != 0) j = (j + 1) & ngmask;
      sig_ok = ngs[j].sig == sig && ngs[j].prob == sl.prob && ngs[j].backoff == sl.backoff;
      if (sig_ok && sl.n == 1) sig_ok = uni[sl.ids[0]].prob == sl.prob && uni[sl.ids[0]].backoff == sl.backoff;
      if (sig_ok && sl.n >= 2) {
        const uint64_t bit = 1ULL << cont_bit(sl.ids[sl.n - 1]);
        const NgSlot* c = lm_ngram_find(hv, sl.ids, sl.n - 1);
        const uint64_t cont = sl.n == 2 ? uni[sl.ids[0]].cont : (c ? ngs[(size_t)(c - lm->ng.data())].cont : 0ULL);
        sig_ok = (sl.n == 2 || c) && (cont & bit) != 0;         // (an unlisted context fails: the kernel would never probe the n-gram)
      }
    }
    if (!sig_ok) fprintf(stderr, "e2e_lm: the kernel's tables failed their self-check; using the id tables (slower)\n");
  }
  if (getenv("E2E_LM_DEBUG")) fprintf(stderr, "e2e_lm: %zu entries, %zu words, signature tables %s\n", entries.size(), words.size(), sig_ok ? "ok" : "NOT usable");
  bool ok = (!sig_ok || up((void**)&lm->d_ngs, ngs.data(), ngs.size() * sizeof(NgSig))) &&
            up((void**)&lm->d_vt, vt.data(), vt.size() * sizeof(VEntry)) &&
            up((void**)&lm->d_uni, uni.data(), uni.size() * sizeof(UniEntry)) &&
            up((void**)&lm->d_vkeys, lm->vkeys.data(), lm->vkeys.size() * sizeof(uint64_t)) &&
            up((void**)&lm->d_vvals, lm->vvals.data(), lm->vvals.size() * sizeof(uint32_t)) &&
            up((void**)&lm->d_ng, lm->ng.data(), lm->ng.size() * sizeof(NgSlot)) &&
            up((void**)&lm->d_label_bytes, lm->label_bytes.data(), lm->label_bytes.size()) &&
            up((void**)&lm->d_label_off, lm->label_off.data(), lm->label_off.size() * sizeof(int)) &&
            (lm->homs.empty() || up((void**)&lm->d_homs, lm->homs.data(), lm->homs.size() * sizeof(uint32_t)));
  if (!ok) {
    // no usable GPU: keep the host tables (e2e_lm_word_index / e2e_lm_score still work); e2e_ctc_beam refuses it
    (void)hipGetLastError();
    (void)hipFree(lm->d_vkeys); (void)hipFree(lm->d_vvals); (void)hipFree(lm->d_ng);
    (void)hipFree(lm->d_label_bytes); (void)hipFree(lm->d_label_off); (void)hipFree(lm->d_ngs); (void)hipFree(lm->d_vt); (void)hipFree(lm->d_uni);
    (void)hipFree(lm->d_homs); lm->d_homs = nullptr;
    lm->d_vkeys = nullptr; lm->d_vvals = nullptr; lm->d_ng = nullptr; lm->d_label_bytes = nullptr; lm->d_label_off = nullptr;
    lm->d_ngs = nullptr; lm->d_vt = nullptr; lm->d_uni = nullptr;
  } else if (hipGetDevice(&lm->device) != hipSuccess) {
    lm->device = -1;
  }
}

extern "C" void e2e_lm_free(e2e_lm* lm) {
  if (!lm) return;
  (void)hipFree(lm->d_vkeys); (void)hipFree(lm->d_vvals); (void)hipFree(lm->d_ng);
  (void)hipFree(lm->d_label_bytes); (void)hipFree(lm->d_label_off); (void)hipFree(lm->d_ngs); (void)hipFree(lm->d_vt); (void)hipFree(lm->d_uni);
  (void)hipFree(lm->d_homs);
  delete lm;
}

extern "C" int e2e_lm_order(const e2e_lm* lm) { return lm ? lm->order : 0; }
extern "C" int e2e_lm_device(const e2e_lm* lm) { return lm ? lm->device : -1; }

int e2e::check_model_device(const e2e_lm* lm) {
  if (!lm) return E2E_OK;
  if (!lm->d_ng) { set_error("the language model has no device tables (it was loaded without a GPU)"); return E2E_ERR_HIP; }
  int cur = -1;
  E2E_HIP_CHECK(hipGetDevice(&cur), "hipGetDevice");
  if (cur != lm->device) {
    set_error("the language model's tables are on device %d but the call runs on device %d: load it once per device", lm->device, cur);
    return E2E_ERR_ARG;
  }
  return E2E_OK;
}

int e2e::check_lexicon(const e2e_lm* lm, bool restricted) {
  if (!restricted || (lm && lm->has_lexicon)) return E2E_OK;
  set_error(lm ? "restrict_to_lexicon: the model has no lexicon (e2e_lm_enable_lexicon)" : "restrict_to_lexicon needs a model: a language model or a word list (e2e_lm_load_words)");
  return E2E_ERR_ARG;
}

int e2e::check_row_bytes(size_t row_bytes, size_t want, const char* query) {
  if (row_bytes >= want && row_bytes % 8 == 0) return E2E_OK;
  set_error("row_bytes = %zu: a state row needs %zu bytes (%s) and a multiple of 8", row_bytes, want, query);
  return E2E_ERR_ARG;
}

int e2e::check_state_aligned(int B, const void* state) {
  if (B <= 0 || reinterpret_cast<uintptr_t>(state) % 8 == 0) return E2E_OK;
  set_error("the state must be 8-byte aligned");
  return E2E_ERR_ARG;
}

// get_idx(string), ctc_decoder.cpp:77-82: exact lookup when case sensitive, else lower-cased lookup
extern "C" uint32_t e2e_lm_word_index(const e2e_lm* lm, const char* word) {
  if (!lm || !word) return 0;
  const std::string w = lm->fold_case ? lower(word) : std::string(word);
  if (lm->transcribed) {                                   // (the vocabulary table is keyed by transcriptions)
    auto it = lm->folded.find(w);
    return it == lm->folded.end() ? 0u : it->second;
  }
  return lm_word_lookup(lm->host_view(), word_hash(w));
}

extern "C" double e2e_lm_score(const e2e_lm* lm, const uint32_t* ctx, int ctx_len, uint32_t word) {
  if (!lm || ctx_len < 0 || ctx_len > kCtx || (ctx_len > 0 && !ctx)) return 0.0;
  return (double)lm_base_score(lm->host_view(), ctx, ctx_len, word, nullptr, nullptr);
}

// A model that scores nothing, from a word list: order 1, every word and <unk> at log10 p = 0.  It exists so that a search can
// be restricted to a lexicon without a language model (e2e_lm_enable_lexicon): with the restriction off, lmwt anything and
// oov_penalty = 0, its search is the search without a model.
extern "C" int e2e_lm_load_words(const char* const* words_in, int n_words, const char* const* labels, int V, int case_sensitive,
                                 e2e_lm** out) {
  if (out) *out = nullptr;
  if (!out || n_words < 0 || (n_words > 0 && !words_in) || V < 0 || (V > 0 && !labels)) { set_error("e2e_lm_load_words: bad argument"); return E2E_ERR_ARG; }
  for (int i = 0; i < n_words; i++) {
    const char* w = words_in[i];
    if (!w || !*w || strpbrk(w, " \t\r\n")) { set_error("e2e_lm_load_words: entry %d is empty or holds white space", i); return E2E_ERR_ARG; }
  }
  e2e_lm* lm = new e2e_lm();
  lm->fold_case = case_sensitive ? 0 : 1;
  lm->order = 1;
  lm->words_only = true;
  std::vector<std::string> words;
  std::vector<Entry> entries;
  auto add = [&](const std::string& w) {
    if (!lm->exact.emplace(w, (uint32_t)words.size()).second) return;        // (listed twice: once)
    Entry e; e.n = 1; e.ids[0] = (uint32_t)words.size(); e.prob = 0.f; e.bo = 0.f;
    words.push_back(w); entries.push_back(e);
  };
  add("<unk>"); add("<s>"); add("</s>");
  for (int i = 0; i < n_words; i++) add(words_in[i]);
  build_model(lm, words, entries, labels, V);
  *out = lm;
  return E2E_OK;
}

extern "C" int e2e_lm_has_lexicon(const e2e_lm* lm) { return lm && lm->has_lexicon ? 1 : 0; }

// bit 0: the spelling is a word of the lexicon; bit 1: it is a proper prefix of a longer word.  0 without a lexicon.
extern "C" int e2e_lm_spelling_class(const e2e_lm* lm, const char* spelling) {
  if (!lm || !spelling || !lm->has_lexicon || lm->transcribed) return 0;
  auto it = lm->lex_class.find(lm->fold_case ? lower(spelling) : std::string(spelling));
  return it == lm->lex_class.end() ? 0 : it->second;
}

// The lexicon of a model: its words (the unigrams but <unk>, <s>, </s>) as the LM lookup spells them, and their prefixes.  The
// prefixes that are no words enter the vocabulary tables -- the id table and the kernel's two-choice table -- with id 0 and
// <unk>'s unigram: every lookup that is not restricted reads them as the miss they were, and the one probe a restricted search
// makes for a word's id also tells it whether the spelling may go on.  Allocates and synchronises, like the loader.
extern "C" int e2e_lm_enable_lexicon(e2e_lm* lm) {
  if (!lm) { set_error("e2e_lm_enable_lexicon: no model"); return E2E_ERR_ARG; }
  if (lm->has_lexicon) return E2E_OK;
  const LmView hv = lm->host_view();
  std::unordered_map<std::string, unsigned char> cls;
  std::vector<std::string> prefixes;                       // proper prefixes that are no words
  // (a transcription model: L is the kept transcriptions, as id codes, and a prefix ends on a label boundary)
  const size_t unit = lm->transcribed ? 2 : 1;
  if (lm->transcribed) for (const auto& k : lm->tr_keys) cls[k] |= 1;
  else for (const auto& kv : lm->exact) {
    if (is_special(kv.first)) continue;
    cls[lm->fold_case ? lower(kv.first) : kv.first] |= 1;
  }
  {
    std::vector<std::string> ws;
    for (const auto& kv : cls) ws.push_back(kv.first);
    for (const auto& w : ws)
      for (size_t n = unit; n < w.size(); n += unit) {
        unsigned char& c = cls[w.substr(0, n)];
        if (c == 0) prefixes.push_back(w.substr(0, n));
        c |= 2;
      }
  }
  // <unk>, <s> and </s> stay in the tables (an unrestricted search may spell and find them) but are no words of the lexicon.
  // The tables cannot say so, so a model whose labels can spell one of them inside the lexicon is refused: some chain of
  // labels spells it with every label boundary on the way at an allowed spelling.
  const int V = (int)lm->label_off.size() - 1;
  auto label = [&](int c) {
    std::string s((const char*)lm->label_bytes.data() + lm->label_off[c], (size_t)(lm->label_off[c + 1] - lm->label_off[c]));
    return lm->fold_case ? lower(s) : s;
  };
  // (A transcription model cannot spell them at all: they have no transcription.)
  for (const char* sp : {"<unk>", "<s>", "</s>"}) {
    const std::string s = sp;
    if (lm->transcribed) break;
    if (!lm->exact.count(s) && !(lm->fold_case && lm_word_lookup(hv, word_hash(s)))) continue;
    std::vector<char> reach(s.size() + 1, 0);
    reach[0] = 1;
    for (size_t o = 0; o < s.size(); o++) {
      if (!reach[o] || (o > 0 && !cls.count(s.substr(0, o)))) continue;
      for (int c = 0; c < V; c++) {
        const std::string l = label(c);
        if (!l.empty() && s.compare(o, l.size(), l) == 0 && o + l.size() <= s.size()) reach[o + l.size()] = 1;
      }
    }
    if (reach[s.size()]) {
      set_error("e2e_lm_enable_lexicon: the labels can spell %s, which the tables could not tell from a word", sp);
      return E2E_ERR_UNSUPPORTED;
    }
  }
  // the id table again, with room for the prefixes; then the kernel's table of the same size (they share vmask)
  std::vector<uint64_t> vkeys; std::vector<uint32_t> vvals; std::vector<VEntry> vt;
  const bool want_vt = lm->d_ngs != nullptr || lm->device < 0;
  size_t old_n = 0;
  for (uint64_t k : lm->vkeys) old_n += k != 0;
  bool built = false;
  for (size_t size = pow2_at_least((old_n + prefixes.size()) * 4 + 16), tries = 0; tries < 4 && !built; size *= 2, tries++) {
    if (size < lm->vkeys.size()) size = lm->vkeys.size();
    vkeys.assign(size, 0); vvals.assign(size, 0);
    const uint32_t vmask = (uint32_t)size - 1;
    auto put = [&](uint64_t h, uint32_t id) {
      for (uint32_t i = (uint32_t)h & vmask;; i = (i + 1) & vmask) {
        if (vkeys[i] == h) return;                         // (a word's entry stands: words go in first)
        if (vkeys[i] == 0) { vkeys[i] = h; vvals[i] = id; return; }
      }
    };
    for (size_t i = 0; i < lm->vkeys.size(); i++) if (lm->vkeys[i]) put(lm->vkeys[i], lm->vvals[i]);
    for (const auto& s : prefixes) put(word_hash(s), 0u);
    built = true;
    if (!want_vt) break;
    vt.assign(size, VEntry{0, 0u, 1.f});
    for (size_t i = 0; i < size && built; i++) {
      if (vkeys[i] == 0) continue;
      const NgSlot* u = lm_ngram_find(hv, &vvals[i], 1);
      built = cuckoo_insert(vt, VEntry{vkeys[i], vvals[i], u ? u->prob : 1.f});
    }
    for (size_t i = 0; i < size && built; i++) {           // self-check, as the loader's
      if (vkeys[i] == 0) continue;
      uint32_t i1, i2;
      two_slots(vkeys[i], vmask, i1, i2);
      const VEntry* e = vt[i1].key == vkeys[i] ? &vt[i1] : vt[i2].key == vkeys[i] ? &vt[i2] : nullptr;
      built = e && e->val == vvals[i];
    }
  }
  if (!built) { set_error("e2e_lm_enable_lexicon: the two-choice vocabulary table could not be built"); return E2E_ERR_UNSUPPORTED; }
  if (getenv("E2E_LM_DEBUG"))
    fprintf(stderr, "e2e_lm lexicon: %zu spellings, %zu of them prefixes only; vocabulary tables %zu -> %zu bytes\n", cls.size(),
            prefixes.size(), lm->vkeys.size() * (12 + sizeof(VEntry)), vkeys.size() * (12 + sizeof(VEntry)));
  if (lm->device >= 0) {
    int cur = -1;
    E2E_HIP_CHECK(hipGetDevice(&cur), "hipGetDevice");
    E2E_HIP_CHECK(hipSetDevice(lm->device), "hipSetDevice");
    uint64_t* dk = nullptr; uint32_t* dv = nullptr; VEntry* dt = nullptr;
    const bool ok = upload((void**)&dk, vkeys.data(), vkeys.size() * sizeof(uint64_t)) &&
                    upload((void**)&dv, vvals.data(), vvals.size() * sizeof(uint32_t)) &&
                    upload((void**)&dt, vt.data(), vt.size() * sizeof(VEntry)) &&
                    hipDeviceSynchronize() == hipSuccess;       // (nothing in flight reads the tables that are freed below)
    if (!ok) {
      (void)hipGetLastError();
      (void)hipFree(dk); (void)hipFree(dv); (void)hipFree(dt);
      (void)hipSetDevice(cur);
      set_error("e2e_lm_enable_lexicon: the tables could not be uploaded");
      return E2E_ERR_HIP;
    }
    (void)hipFree(lm->d_vkeys); (void)hipFree(lm->d_vvals); (void)hipFree(lm->d_vt);
    lm->d_vkeys = dk; lm->d_vvals = dv; lm->d_vt = dt;
    (void)hipSetDevice(cur);
  }
  lm->vkeys.swap(vkeys); lm->vvals.swap(vvals);
  lm->lex_class.swap(cls);
  lm->has_lexicon = true;
  return E2E_OK;
}

// ------------------------------------------------------------------------------------------------------
// custom transcriptions (a pronunciation lexicon), homophones included: the definition is in DESIGN.md 4.4
// ------------------------------------------------------------------------------------------------------
extern "C" int e2e_lm_is_transcribed(const e2e_lm* lm) { return lm && lm->transcribed ? 1 : 0; }
extern "C" int e2e_lm_transcriptions_dropped(const e2e_lm* lm) { return lm ? lm->transcriptions_dropped : 0; }
extern "C" const char* e2e_lm_word_string(const e2e_lm* lm, uint32_t id) {
  return lm && id < lm->words.size() ? lm->words[id].c_str() : nullptr;
}

extern "C" int e2e_lm_load_transcriptions(const char* path, const char* const* entry_words, const int32_t* entry_label_ids,
                                          const int32_t* entry_off, int n_entries, const char* const* labels, int V,
                                          int case_sensitive, e2e_lm** out) {
  if (out) *out = nullptr;
  if (!out || n_entries < 0 || V < 1 || !labels || (n_entries > 0 && (!entry_words || !entry_off || !entry_label_ids))) {
    set_error("e2e_lm_load_transcriptions: bad argument");
    return E2E_ERR_ARG;
  }
  if (n_entries == 0) { set_error("e2e_lm_load_transcriptions: the lexicon is empty"); return E2E_ERR_ARG; }
  if (V > 65535) { set_error("e2e_lm_load_transcriptions: %d labels: a label's code has two bytes, at most 65535", V); return E2E_ERR_UNSUPPORTED; }
  // every entry's form, before anything is loaded
  for (int i = 0; i < n_entries; i++) {
    const char* w = entry_words[i];
    if (!w || !*w || strpbrk(w, " \t\r\n")) { set_error("e2e_lm_load_transcriptions: entry %d: the word is empty or holds white space", i); return E2E_ERR_ARG; }
    if (is_special(w)) { set_error("e2e_lm_load_transcriptions: entry %d: %s has no transcription", i, w); return E2E_ERR_ARG; }
    const int64_t k = (int64_t)entry_off[i + 1] - entry_off[i];
    if (entry_off[i] < 0 || k < 1) { set_error("e2e_lm_load_transcriptions: entry %d (%s) has no labels", i, w); return E2E_ERR_ARG; }
    if (k > kMaxTranscription) {
      set_error("e2e_lm_load_transcriptions: entry %d (%s) has %lld labels: at most %d", i, w, (long long)k, kMaxTranscription);
      return E2E_ERR_UNSUPPORTED;
    }
    for (int j = entry_off[i]; j < entry_off[i + 1]; j++) {
      const int c = entry_label_ids[j];
      if (c < 0 || c >= V) { set_error("e2e_lm_load_transcriptions: entry %d (%s): %d is no label id (V = %d)", i, w, c, V); return E2E_ERR_ARG; }
      if (strcmp(labels[c], " ") == 0) { set_error("e2e_lm_load_transcriptions: entry %d (%s): the space is the word boundary and no token", i, w); return E2E_ERR_ARG; }
    }
  }
  std::vector<std::string> words;
  std::vector<Entry> entries;
  e2e_lm* lm = nullptr;
  if (path) {
    const int rc = read_arpa(path, case_sensitive, &lm, words, entries);
    if (rc != E2E_OK) return rc;
  } else {                                                 // the model that scores nothing (e2e_lm_load_words) over the entries' words
    lm = new e2e_lm();
    lm->fold_case = case_sensitive ? 0 : 1;
    lm->order = 1;
    auto add = [&](const std::string& w) {
      if (!lm->exact.emplace(w, (uint32_t)words.size()).second) return;
      Entry e; e.n = 1; e.ids[0] = (uint32_t)words.size(); e.prob = 0.f; e.bo = 0.f;
      words.push_back(w); entries.push_back(e);
    };
    add("<unk>"); add("<s>"); add("</s>");
    for (int i = 0; i < n_entries; i++) add(entry_words[i]);
  }
  for (uint32_t id = 0; id < words.size(); id++)           // (two words that fold to one string: the lowest id, as build_model)
    lm->folded.emplace(lm->fold_case ? lower(words[id]) : words[id], id);
  std::vector<TrKey> keys;
  std::unordered_map<std::string, size_t> at;              // code -> index in keys
  std::unordered_map<uint64_t, size_t> by_hash;
  for (int i = 0; i < n_entries; i++) {
    const std::string w = lm->fold_case ? lower(entry_words[i]) : std::string(entry_words[i]);
    auto it = lm->folded.find(w);
    if (it == lm->folded.end() || is_special(words[it->second])) { lm->transcriptions_dropped++; continue; }
    std::string code;
    for (int j = entry_off[i]; j < entry_off[i + 1]; j++) {
      const int c = entry_label_ids[j] + 1;
      code.push_back((char)(c & 255)); code.push_back((char)(c >> 8));
    }
    auto ins = at.emplace(code, keys.size());
    if (ins.second) {
      const uint64_t h = word_hash(code);
      if (!by_hash.emplace(h, keys.size()).second) {
        delete lm;
        set_error("e2e_lm_load_transcriptions: entry %d (%s): its transcription shares a 64-bit hash with another", i, entry_words[i]);
        return E2E_ERR_UNSUPPORTED;
      }
      keys.push_back(TrKey{code, h, {}});
    }
    std::vector<uint32_t>& ids = keys[ins.first->second].ids;
    if (std::find(ids.begin(), ids.end(), it->second) != ids.end()) continue;        // (listed twice: once)
    if ((int)ids.size() == kMaxHomophones) {
      delete lm;
      set_error("e2e_lm_load_transcriptions: entry %d (%s): more than %d words share its transcription", i, entry_words[i], kMaxHomophones);
      return E2E_ERR_UNSUPPORTED;
    }
    ids.push_back(it->second);
  }
  for (const TrKey& k : keys) lm->tr_keys.push_back(k.code);
  build_model(lm, words, entries, labels, V, &keys);
  *out = lm;
  return E2E_OK;
}

// The words of a label sequence, as a search over this model reads them: split at the space (empty pieces skipped), each
// piece looked up as the kernel spells it, a homophone set resolved in the running context (lm_homophone_choice).  A piece
// that is no key is <unk> (0).  Writes at most max_words ids; *n_words is the number of pieces.
extern "C" int e2e_lm_transcribe(const e2e_lm* lm, const int64_t* ids, int64_t n, int space_id, uint32_t* word_ids_out,
                                 int max_words, int* n_words) {
  if (n_words) *n_words = 0;
  if (!lm || n < 0 || (n > 0 && !ids) || max_words < 0 || (max_words > 0 && !word_ids_out) || !n_words) {
    set_error("e2e_lm_transcribe: bad argument");
    return E2E_ERR_ARG;
  }
  const int V = (int)lm->label_off.size() - 1;
  for (int64_t i = 0; i < n; i++)
    if (ids[i] < 0 || ids[i] >= V) { set_error("e2e_lm_transcribe: id %lld at %lld is no label (V = %d)", (long long)ids[i], (long long)i, V); return E2E_ERR_ARG; }
  const LmView hv = lm->host_view();
  uint32_t ctx[kLmMaxOrder] = {lm->bos}; int ctx_len = 1;
  int count = 0;
  for (int64_t i = 0; i < n;) {
    if (ids[i] == space_id) { i++; continue; }
    uint64_t h = kFnvInit;
    for (; i < n && ids[i] != space_id; i++)
      for (int b = lm->label_off[ids[i]]; b < lm->label_off[ids[i] + 1]; b++) {
        unsigned char ch = lm->label_bytes[b];
        if (hv.fold_case && ch >= 'A' && ch <= 'Z') ch += 32;
        h = fnv_step(h, ch);
      }
    uint32_t w = lm_word_lookup(hv, h);
    if (is_hom_ref(w)) { float sc; w = lm_homophone_choice(hv, w, ctx, ctx_len, &sc); }
    uint32_t next[kLmMaxOrder]; int next_len = 0;
    (void)lm_base_score(hv, ctx, ctx_len, w, next, &next_len);
    for (int k = 0; k < next_len; k++) ctx[k] = next[k];
    ctx_len = next_len;
    if (count < max_words) word_ids_out[count] = w;
    count++;
  }
  *n_words = count;
  return E2E_OK;
}
