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

}  // namespace
}  // namespace e2e

using namespace e2e;

extern "C" int e2e_lm_load_arpa(const char* path, const char* const* labels, int V, int case_sensitive, e2e_lm** out) {
  if (out) *out = nullptr;
  if (!path || !out || V < 0 || (V > 0 && !labels)) { set_error("e2e_lm_load_arpa: bad argument"); return E2E_ERR_ARG; }
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
  std::vector<std::string> words;                          // id -> word; id 0 is <unk>
  auto intern = [&](const std::string& w) -> uint32_t {
    auto it = lm->exact.find(w);
    if (it != lm->exact.end()) return it->second;
    const uint32_t id = (uint32_t)words.size();
    words.push_back(w); lm->exact.emplace(w, id);
    return id;
  };
  intern("<unk>");
  struct Entry { uint32_t ids[kLmMaxOrder]; int n; float prob, bo; };
  std::vector<Entry> entries;
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
  lm->vkeys.assign(pow2_at_least(words.size() * 4 + 16), 0);
  lm->vvals.assign(lm->vkeys.size(), 0);
  const uint32_t vmask = (uint32_t)lm->vkeys.size() - 1;
  for (uint32_t id = 0; id < words.size(); id++) {
    const uint64_t h = word_hash(lm->fold_case ? lower(words[id]) : words[id]);
    for (uint32_t i = (uint32_t)h & vmask;; i = (i + 1) & vmask) {
      if (lm->vkeys[i] == h) break;
      if (lm->vkeys[i] == 0) { lm->vkeys[i] = h; lm->vvals[i] = id; break; }
    }
  }
  { auto it = lm->exact.find("<s>"); lm->bos = it != lm->exact.end() ? it->second : 0; }
  lm->label_off.assign(1, 0);
  for (int c = 0; c < V; c++) {
    for (const char* s = labels[c]; *s; s++) lm->label_bytes.push_back((unsigned char)*s);
    lm->label_off.push_back((int)lm->label_bytes.size());
  }
  if (lm->label_bytes.empty()) lm->label_bytes.push_back(0);
  // upload
  auto up = [](void** d, const void* h, size_t bytes) -> bool {
    if (hipMalloc(d, bytes) != hipSuccess) return false;
    return hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice) == hipSuccess;
  };
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
    // cuckoo insertion: a free slot of the item's two, else evict the occupant of one and move that on
    VEntry item{lm->vkeys[i], lm->vvals[i], uni[lm->vvals[i]].prob};
    const uint32_t mask = (uint32_t)vt.size() - 1;
    uint32_t i1, i2;
    two_slots(item.key, mask, i1, i2);
    if (vt[i1].key == 0) { vt[i1] = item; continue; }
    if (vt[i2].key == 0) { vt[i2] = item; continue; }
    uint32_t pos = i1;
    bool placed = false;
    for (int kick = 0; kick < 2000 && !placed; kick++) {
      std::swap(item, vt[pos]);
      if (item.key == 0) { placed = true; break; }
      two_slots(item.key, mask, i1, i2);
      pos = pos == i1 ? i2 : i1;
    }
    if (!placed) sig_ok = false;                                  // (never seen at load <= 1/4; the id-keyed walk takes over)
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
      sig_ok = e && e->val == lm->vvals[i] && e->prob == uni[e->val].prob;
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
            up((void**)&lm->d_label_off, lm->label_off.data(), lm->label_off.size() * sizeof(int));
  if (!ok) {
    // no usable GPU: keep the host tables (e2e_lm_word_index / e2e_lm_score still work); e2e_ctc_beam refuses it
    (void)hipGetLastError();
    (void)hipFree(lm->d_vkeys); (void)hipFree(lm->d_vvals); (void)hipFree(lm->d_ng);
    (void)hipFree(lm->d_label_bytes); (void)hipFree(lm->d_label_off); (void)hipFree(lm->d_ngs); (void)hipFree(lm->d_vt); (void)hipFree(lm->d_uni);
    lm->d_vkeys = nullptr; lm->d_vvals = nullptr; lm->d_ng = nullptr; lm->d_label_bytes = nullptr; lm->d_label_off = nullptr;
    lm->d_ngs = nullptr; lm->d_vt = nullptr; lm->d_uni = nullptr;
  } else if (hipGetDevice(&lm->device) != hipSuccess) {
    lm->device = -1;
  }
  *out = lm;
  return E2E_OK;
}

extern "C" void e2e_lm_free(e2e_lm* lm) {
  if (!lm) return;
  (void)hipFree(lm->d_vkeys); (void)hipFree(lm->d_vvals); (void)hipFree(lm->d_ng);
  (void)hipFree(lm->d_label_bytes); (void)hipFree(lm->d_label_off); (void)hipFree(lm->d_ngs); (void)hipFree(lm->d_vt); (void)hipFree(lm->d_uni);
  delete lm;
}

extern "C" int e2e_lm_order(const e2e_lm* lm) { return lm ? lm->order : 0; }
extern "C" int e2e_lm_device(const e2e_lm* lm) { return lm ? lm->device : -1; }

// get_idx(string), ctc_decoder.cpp:77-82: exact lookup when case sensitive, else lower-cased lookup
extern "C" uint32_t e2e_lm_word_index(const e2e_lm* lm, const char* word) {
  if (!lm || !word) return 0;
  const std::string w = lm->fold_case ? lower(word) : std::string(word);
  return lm_word_lookup(lm->host_view(), word_hash(w));
}

extern "C" double e2e_lm_score(const e2e_lm* lm, const uint32_t* ctx, int ctx_len, uint32_t word) {
  if (!lm || ctx_len < 0 || ctx_len > kCtx || (ctx_len > 0 && !ctx)) return 0.0;
  return (double)lm_base_score(lm->host_view(), ctx, ctx_len, word, nullptr, nullptr);
}
