// Prefix beam search with optional n-gram LM scoring: the host side.  The algorithm, the types and the phases the kernels share
// are in ctc_beam_common.h, the kernels in ctc_beam_lds.hip (the beam in LDS) and ctc_beam_general.hip (any alphabet width), one
// object per input dtype each.  Here: the LDS layouts, which kernel a call takes (beam_fits / gen_fits / beam_takes_general) and
// which of its instances (lmk_of, kernel_of); what a call's workspace holds and where (beam_plan: the queries' and the call's);
// and the C entry points of include/e2e_ctc.h, each of which fills a BeamArgs and calls beam_run.
#include <cstdio>
#include <cstring>

#include <stdlib.h>

#include "ctc_beam_common.h"

using namespace e2e;
using namespace e2e::beamk;

struct GenLayout { size_t gkey, lmc, gmem, total, lds, gstride; int CH; bool members_in_ws; };
// (K1 > 0: a pruned call -- K1 candidates per member instead of V, no LM answer rows)
static GenLayout gen_layout(int B, int V, int W, int WP2, int HS, bool lm, int K1 = 0) {
  GenLayout l;
  l.CH = 256; while (l.CH < 4 * W) l.CH <<= 1;
  size_t o = 0;
  l.gstride = (size_t)W + (size_t)W * (K1 > 0 ? K1 : V);
  l.gkey = o; o += align_up((size_t)B * l.gstride * sizeof(unsigned long long), 256);
  l.lmc = o; if (lm && K1 <= 0) o += align_up((size_t)B * 2 * (size_t)W * V * sizeof(LmAnswer), 256);
  l.gmem = o; o += align_up((size_t)B * 2 * Members::bytes(W), 256);       // (used only when the member sets leave LDS)
  l.total = o;
  const size_t rest = (sizeof(unsigned long long) + sizeof(double) + sizeof(int)) * (size_t)(WP2 + 8) +
          sizeof(int) * (kSelBins + 64 + 4 * (size_t)HS + 4 * (size_t)l.CH + (size_t)gen_list_cap(W) + (size_t)gen_bitmap_words(V)) + 64;
  l.members_in_ws = rest + 2 * Members::bytes(W) > (size_t)kLdsBudget;
  l.lds = rest + (l.members_in_ws ? 0 : 2 * Members::bytes(W));
  return l;
}

struct BeamLayout { size_t nodes, total, lds; int NCAP, CMAX, WP2, HS; };
static BeamLayout beam_layout(int B, int T, int V, int W, bool lm = false) {
  BeamLayout l;
  l.CMAX = W * V + W + 8;
  // live nodes: the beam and its ancestors (at most one root path of length <= T per member); at most W are created per step
  l.NCAP = W * (T + 3) + 8;
  l.WP2 = 64; while (l.WP2 < W) l.WP2 <<= 1;
  l.HS = 256; while (l.HS < 4 * W) l.HS <<= 1;
  l.lds = BeamLds::bytes(W, V, l.CMAX, l.WP2, l.HS, lm);
  size_t o = 0;
  l.nodes = o; o += align_up((size_t)B * l.NCAP * sizeof(BeamNode), 256);
  l.total = o;
  return l;
}

// The instance a call launches: the object of its dtype hands out its kernel for (lmk, st).
// (16-bit log-probabilities are read as they are -- every one of them is an f32 number, so the search is the f32 one's, bit for bit)
template <typename IO> static const void* kernel_of_io(bool general, int lmk, bool st, bool cut) {
  return !general ? lds_kernel<IO>(lmk, st) : cut ? general_kernel<IO, true>(lmk, st) : general_kernel<IO, false>(lmk, st);
}
static const void* kernel_of(int dtype, bool general, int lmk, bool st, bool cut = false) {
  switch (dtype) {
    case E2E_F32: return kernel_of_io<float>(general, lmk, st, cut);
    case E2E_F64: return kernel_of_io<double>(general, lmk, st, cut);
    case E2E_F16: return kernel_of_io<f16_t>(general, lmk, st, cut);
    default:      return kernel_of_io<bf16_t>(general, lmk, st, cut);     // (check_args has checked the dtype)
  }
}

// does one workgroup's LDS hold the beam of this width over this alphabet? (the fast kernel)
static bool beam_fits(int V, int W, bool lm) {
  if (V < 1 || W < 1) return false;
  if ((long long)W * V + W + 8 > kMaxCand || W > kSelBins) return false;
  if (lm && 2 * W > kStateSlots) return false;
  const BeamLayout l = beam_layout(1, 1, V, W, lm);
  return l.lds <= (size_t)kLdsBudget;
}
// ... the general kernel (everything that scales with the alphabet is in the workspace)
static bool gen_fits(int V, int W, bool lm) {
  if (V < 1 || W < 1 || W > kGenMaxW || (long long)W * V > 0x7fffffffLL / 2) return false;
  const BeamLayout l = beam_layout(1, 1, V, W, lm);
  return gen_layout(1, V, W, l.WP2, l.HS, lm).lds <= (size_t)kLdsBudget;
}

extern "C" int e2e_ctc_beam_max_width(int V, int with_lm) {
  if (V < 1) return 0;
  int lo = 0, hi = kSelBins;                    // the largest supported width (the tests are monotone in the width)
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (beam_fits(V, mid, with_lm != 0) || gen_fits(V, mid, with_lm != 0)) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// which kernel a call takes
static bool beam_takes_general(int V, int W, bool lm) {
  static const bool force_general = getenv("E2E_BEAM_GENERAL") != nullptr;      // (tests: the whole suite through the general kernel)
  const bool fast_ok = beam_fits(V, W, lm), gen_ok = gen_fits(V, W, lm);
  return gen_ok && (!fast_ok || force_general);
}

extern "C" int e2e_ctc_beam_cut_max_width(int V, int with_lm) {
  if (V < 1) return 0;
  int lo = 0, hi = kGenMaxW;                    // (a pruned call always takes the general kernel)
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (gen_fits(V, mid, with_lm != 0)) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---- what a call adds to the arguments of e2e_ctc_beam (each null: the call without it) ----
// e2e_ctc_beam_nbest: the n-best read-out
struct NBestOut { int nbest; int64_t* n_hyp; double* scores; int32_t* counts; int64_t* timesteps; };
// e2e_ctc_beam_stream: the state rows
struct StreamIn { void* state; size_t row_bytes; int max_frames, with_timesteps; int64_t* frames_done; };
// e2e_ctc_beam_nbest_cut / e2e_ctc_beam_stream_cut: the per-frame label pruning
struct CutIn { int top_n; double prob; };
static bool cut_prunes(int V, int top_n, double prob) { return top_n < V || prob < 1.0; }

// the frames' label lists of a pruned call: ids (B,T,K+1) then the counts (B,T), each 256-aligned, written by the selection
// kernel ahead of the search on the stream
struct CutLists { size_t ids, n, total; int K1; };
static CutLists cut_lists(int B, int T, int V, int top_n) {
  CutLists c;
  c.K1 = label_cut_k(V, top_n) + 1;
  c.ids = 0; c.n = align_up((size_t)B * T * c.K1 * sizeof(int), 256);
  c.total = c.n + align_up((size_t)B * T * sizeof(int), 256);
  return c;
}

// a state row: header | one member set | node pool of max_frames frames | the nodes' frames (with_timesteps), each 256-aligned
struct StreamLayout { size_t nodes, frames, total; };
static StreamLayout stream_layout(int max_frames, int V, int W, bool lm, bool ts) {
  StreamLayout l;
  const size_t ncap = (size_t)beam_layout(1, max_frames, V, W, lm).NCAP;
  l.nodes = kStreamHeaderBytes + align_up(Members::bytes(W), 256);
  l.frames = ts ? l.nodes + align_up(ncap * sizeof(BeamNode), 256) : 0;
  l.total = ts ? l.frames + align_up(ncap * sizeof(int), 256) : l.nodes + align_up(ncap * sizeof(BeamNode), 256);
  return l;
}

extern "C" size_t e2e_ctc_beam_stream_row_bytes(int max_frames, int V, int beam_width, int with_lm, int with_timesteps) {
  if (max_frames < 1 || V < 1 || beam_width < 1 || (long long)beam_width * ((long long)max_frames + 3) + 8 > 0x7fffffffLL) return 0;
  if (beam_width > e2e_ctc_beam_max_width(V, with_lm != 0)) return 0;
  return stream_layout(max_frames, V, beam_width, with_lm != 0, with_timesteps != 0).total;
}

// ---- the workspace of a call: which kernel runs, and what lies where.  The queries and the call both ask here ----
// node pool (a whole call's; a stream keeps its nodes in the row) | the general kernel's share: candidate keys, the LM's answer
// rows (with a model, unpruned), member sets of very wide beams (only when that kernel runs: 6.4 MB per utterance instead of 19
// at V = 8000, W = 100 without a model) | the nodes' frames, one int per node (a whole call with timestamps) | the label lists
// (pruned).  T_nodes: the frames the node pool is sized for (a stream: max_frames); T: the chunk's width, for the label lists;
// top_n: cutoff_top_n, 0 for a call that is not pruned (a pruned one always takes the general kernel).
struct BeamPlan { bool general; BeamLayout l; GenLayout g; CutLists c; size_t gen_at, frames_at, lists_at, total; };
static BeamPlan beam_plan(int B, int T_nodes, int T, int V, int W, bool lm, bool ts, bool stream, int top_n) {
  BeamPlan p;
  p.general = top_n > 0 || beam_takes_general(V, W, lm);
  p.l = beam_layout(B, T_nodes, V, W, lm);
  p.c.ids = p.c.n = p.c.total = 0; p.c.K1 = 0;
  if (top_n > 0) p.c = cut_lists(B, T, V, top_n);
  p.g = gen_layout(B, V, W, p.l.WP2, p.l.HS, lm, p.c.K1);
  p.gen_at = stream ? 0 : p.l.total;
  p.frames_at = p.gen_at + (p.general ? p.g.total : 0);
  p.lists_at = p.frames_at + (ts && !stream ? align_up((size_t)B * p.l.NCAP * sizeof(int), 256) : 0);
  p.total = p.lists_at + p.c.total;
  return p;
}

// the queries: the plan's total and 256 bytes of slack for the call to align the pointer with; 0 for bad sizes
extern "C" size_t e2e_ctc_beam_nbest_workspace_bytes(int B, int T, int V, int beam_width, int with_lm, int with_timesteps) {
  if (B < 0 || T < 1 || V < 1 || beam_width < 1) return 0;
  return beam_plan(B, T, T, V, beam_width, with_lm != 0, with_timesteps != 0, false, 0).total + 256;
}
extern "C" size_t e2e_ctc_beam_workspace_bytes_lm(int B, int T, int V, int beam_width, int with_lm) {
  return e2e_ctc_beam_nbest_workspace_bytes(B, T, V, beam_width, with_lm, 0);
}
// (sized for a call with a language model, which every call without one fits as well)
extern "C" size_t e2e_ctc_beam_workspace_bytes(int B, int T, int V, int beam_width) {
  const size_t a = e2e_ctc_beam_workspace_bytes_lm(B, T, V, beam_width, 1), b = e2e_ctc_beam_workspace_bytes_lm(B, T, V, beam_width, 0);
  return a > b ? a : b;
}
// (0, and no workspace, when the one-workgroup kernel takes the stream)
extern "C" size_t e2e_ctc_beam_stream_workspace_bytes(int B, int V, int beam_width, int with_lm) {
  if (B < 0 || V < 1 || beam_width < 1) return 0;
  const BeamPlan p = beam_plan(B, 1, 1, V, beam_width, with_lm != 0, false, true, 0);
  return p.general ? p.total + 256 : 0;
}
// (cutoff_top_n >= V prunes only with cutoff_prob < 1, which the query does not know: such a call may be the unpruned one)
extern "C" size_t e2e_ctc_beam_cut_workspace_bytes(int B, int T, int V, int beam_width, int with_lm, int with_timesteps,
                                                   int cutoff_top_n) {
  if (B < 0 || T < 1 || V < 1 || beam_width < 1 || cutoff_top_n < 1) return 0;
  const size_t pruned = beam_plan(B, T, T, V, beam_width, with_lm != 0, with_timesteps != 0, false, cutoff_top_n).total + 256;
  const size_t plain = cutoff_top_n >= V ? e2e_ctc_beam_nbest_workspace_bytes(B, T, V, beam_width, with_lm, with_timesteps) : 0;
  return pruned > plain ? pruned : plain;
}
extern "C" size_t e2e_ctc_beam_cut_stream_workspace_bytes(int B, int T, int V, int beam_width, int with_lm, int cutoff_top_n) {
  if (B < 0 || T < 1 || V < 1 || beam_width < 1 || cutoff_top_n < 1) return 0;
  const size_t pruned = beam_plan(B, 1, T, V, beam_width, with_lm != 0, false, true, cutoff_top_n).total + 256;
  const size_t plain = cutoff_top_n >= V ? e2e_ctc_beam_stream_workspace_bytes(B, V, beam_width, with_lm) : 0;
  return pruned > plain ? pruned : plain;
}

// ---- a call ----
// the arguments every entry point has: the input, the search's knobs, the outputs, the workspace
struct BeamArgs {
  const void* lp; int dtype; int64_t sB, sT, sV; const int64_t* x_len; int B, T, V, blank;
  int beam_width, space_id; const e2e_lm* lm; double lmwt, wip, oov_penalty; bool restricted;
  int64_t* out; int64_t max_out; int64_t* out_len;
  void* workspace; size_t workspace_bytes; void* stream;
};
static bool restricted_by(const e2e_ctc_beam_opts* opts) { return opts && opts->restrict_to_lexicon != 0; }

// the width limit: an n-best or stream entry reports it as an argument error, e2e_ctc_beam as unsupported.  (beam_fits and
// gen_fits are monotone in the width -- LDS use only grows with it -- so "above the largest width that fits" is "does not fit")
static int check_width(const BeamArgs& a, bool nbest_entry, bool pruned) {
  const bool lm = a.lm != nullptr;
  const int cap = a.V < 1 ? 0 : pruned ? e2e_ctc_beam_cut_max_width(a.V, lm) : e2e_ctc_beam_max_width(a.V, lm);
  if (a.V < 1 || a.beam_width <= cap) return E2E_OK;
  set_error("beam_width = %d over an alphabet of %d%s: at most %d%s", a.beam_width, a.V, lm ? " with a language model" : "", cap,
            nbest_entry ? "" : " (one workgroup's LDS holds the beam)");
  return nbest_entry ? E2E_ERR_ARG : E2E_ERR_UNSUPPORTED;
}

// Every argument error the host can see, before any launch.  The first error wins, so the order is part of the interface; a step
// in brackets is made only by the calls that have that part (nb: an n-best entry, st: a stream, cut: a _cut entry):
//    1. [cut]        cutoff_top_n, cutoff_prob; a cut that prunes nothing (cut_prunes) is dropped: from here on the unpruned call
//    2. [nb, no st]  restrict_to_lexicon without a model or a lexicon
//    3. [st]         bad sizes: B, T, V, beam_width, max_frames
//    4. [nb]         nbest outside [1, beam_width] (a stream: [0, beam_width]; 0 feeds only)
//    5. [st]         null state, frames_done, chunk_len
//    6. [nb]         null n_hyp, scores, counts, out, out_len (a stream: of a call that reads out)
//    7. [st]         timesteps of a stream opened without them
//    8. [nb]         beam_width over the limit: E2E_ERR_ARG
//    9. [st]         max_frames too long to index, row_bytes, the state's alignment
//   10. [st]         restrict_to_lexicon without a model or a lexicon
//   11.              dtype; bad sizes: B, T, V, beam_width, max_out (a stream that feeds only: max_out is not looked at)
//   12.              blank
//   13.              null lp, x_len, out, out_len (a stream that feeds only: no out, out_len)
//   14.              the model's device, then its alphabet
//   15. [cut]        the label selection's own limits (label_cut_check)
//   16. [no nb]      beam_width over the limit: E2E_ERR_UNSUPPORTED (with nb, step 8 has reported it)
// What is left for beam_run: the workspace's size (E2E_ERR_WORKSPACE), then B = 0 is E2E_OK.
static int check_args(const BeamArgs& a, const NBestOut* nb, const StreamIn* st, const CutIn*& cut) {
  const bool lm = a.lm != nullptr;
  if (cut) {
    if (cut->top_n < 1) { set_error("cutoff_top_n=%d: at least 1", cut->top_n); return E2E_ERR_ARG; }
    if (!(cut->prob > 0.0 && cut->prob <= 1.0)) { set_error("cutoff_prob=%g outside (0, 1]", cut->prob); return E2E_ERR_ARG; }
    if (!cut_prunes(a.V, cut->top_n, cut->prob)) cut = nullptr;
  }
  if (nb && !st) if (const int rc = check_lexicon(a.lm, a.restricted)) return rc;
  if (st && (a.B < 0 || a.T < 1 || a.V < 1 || a.beam_width < 1 || st->max_frames < 1)) { set_error("bad sizes"); return E2E_ERR_ARG; }
  if (nb && (nb->nbest < (st ? 0 : 1) || nb->nbest > a.beam_width)) {
    set_error("nbest=%d outside [%d, beam_width=%d]", nb->nbest, st ? 0 : 1, a.beam_width); return E2E_ERR_ARG;
  }
  if (st && a.B > 0 && (!st->state || !st->frames_done || !a.x_len)) { set_error("null pointer argument"); return E2E_ERR_ARG; }
  const bool feeds_only = st && nb->nbest == 0;
  if (nb && !feeds_only && a.B > 0 && (!nb->n_hyp || !nb->scores || !nb->counts || !a.out || !a.out_len)) { set_error("null pointer argument"); return E2E_ERR_ARG; }
  if (st && !st->with_timesteps && nb->timesteps) { set_error("timesteps asked of a stream that was opened with_timesteps = 0"); return E2E_ERR_ARG; }
  if (nb) if (const int rc = check_width(a, true, cut != nullptr)) return rc;
  if (st) {
    const size_t want = e2e_ctc_beam_stream_row_bytes(st->max_frames, a.V, a.beam_width, lm, st->with_timesteps);
    if (!want) { set_error("max_frames = %d: the node pool of a stream this long cannot be indexed", st->max_frames); return E2E_ERR_ARG; }
    if (const int rc = check_row_bytes(st->row_bytes, want, "e2e_ctc_beam_stream_row_bytes")) return rc;
    if (const int rc = check_state_aligned(a.B, st->state)) return rc;
    if (const int rc = check_lexicon(a.lm, a.restricted)) return rc;
  }
  if (a.dtype != E2E_F32 && a.dtype != E2E_F64 && !dtype_is_16bit(a.dtype)) { set_error("dtype must be E2E_F32, E2E_F64, E2E_F16 or E2E_BF16"); return E2E_ERR_ARG; }
  if (a.B < 0 || a.T < 1 || a.V < 1 || a.beam_width < 1 || (!feeds_only && a.max_out < 1)) { set_error("bad sizes"); return E2E_ERR_ARG; }
  if (a.blank < 0 || a.blank >= a.V) { set_error("blank=%d outside [0,%d)", a.blank, a.V); return E2E_ERR_ARG; }
  if (a.B > 0 && (!a.lp || !a.x_len || ((!a.out || !a.out_len) && !feeds_only))) { set_error("null pointer argument"); return E2E_ERR_ARG; }
  if (const int rc = check_model_device(a.lm)) return rc;
  // the kernel spells words with label_off[0..V]: the model must have been loaded with exactly this alphabet
  if (lm && (int)a.lm->label_off.size() - 1 != a.V) {
    set_error("the language model was loaded with %d labels but the log-probabilities have %d columns",
              (int)a.lm->label_off.size() - 1, a.V);
    return E2E_ERR_ARG;
  }
  if (cut) if (const int rc = label_cut_check(a.dtype, a.B, a.T, a.V, a.blank, cut->top_n, cut->prob)) return rc;
  if (!nb) if (const int rc = check_width(a, false, false)) return rc;
  return E2E_OK;
}

// the one call behind every entry point: the checks, the plan, the parameter blocks, the launch (a pruned call: the label
// selection first)
static int beam_run(const BeamArgs& a, const NBestOut* nb = nullptr, const StreamIn* st = nullptr, const CutIn* cut = nullptr) {
  if (const int rc = check_args(a, nb, st, cut)) return rc;
  const e2e_lm* lm = a.lm;
  const bool feeds_only = st && nb->nbest == 0, ts = nb && nb->timesteps && !feeds_only;
  const BeamPlan plan = beam_plan(a.B, st ? st->max_frames : a.T, a.T, a.V, a.beam_width, lm != nullptr, ts, st != nullptr, cut ? cut->top_n : 0);
  const BeamLayout& l = plan.l;
  const uintptr_t base = reinterpret_cast<uintptr_t>(a.workspace), aligned = (base + 255) & ~(uintptr_t)255;
  if (plan.total && (!a.workspace || a.workspace_bytes < plan.total + (aligned - base))) {
    set_error("workspace too small: need %zu", plan.total + 256); return E2E_ERR_WORKSPACE;
  }
  if (a.B == 0) return E2E_OK;
  char* ws = reinterpret_cast<char*>(aligned);
  BeamParams p;
  p.lp = a.lp; p.sB = a.sB; p.sT = a.sT; p.sV = a.sV; p.x_len = a.x_len;
  p.B = a.B; p.T = a.T; p.V = a.V; p.blank = a.blank; p.W = a.beam_width; p.space_id = a.space_id;
  p.has_lm = lm ? 1 : 0;
  if (lm) p.lm = lm->dev_view(); else memset(&p.lm, 0, sizeof(p.lm));
  p.lmwt = lm ? a.lmwt : 0.0;                     // ctc_decoder.cpp:72-74
  p.wip = a.wip; p.oov = a.oov_penalty;
  p.out = a.out; p.max_out = feeds_only ? 1 : a.max_out; p.out_len = a.out_len;
  p.nodes = st ? nullptr : reinterpret_cast<BeamNode*>(ws + l.nodes);
  p.NCAP = l.NCAP; p.CMAX = l.CMAX; p.WP2 = l.WP2; p.HS = l.HS;
  p.nbest = nb ? nb->nbest : 0;
  p.n_hyp = nb ? nb->n_hyp : nullptr; p.scores = nb ? nb->scores : nullptr; p.counts = nb ? nb->counts : nullptr;
  p.ts_out = ts ? nb->timesteps : nullptr;
  p.node_t = ts && !st ? reinterpret_cast<int*>(ws + plan.frames_at) : nullptr;
  p.st_rows = nullptr; p.st_row_bytes = 0; p.st_nodes_off = 0; p.st_ts_off = 0; p.st_max_frames = 0; p.frames_done = nullptr;
  if (st) {
    const StreamLayout sl = stream_layout(st->max_frames, a.V, a.beam_width, lm != nullptr, st->with_timesteps != 0);
    p.st_rows = static_cast<unsigned char*>(st->state); p.st_row_bytes = st->row_bytes;
    p.st_nodes_off = sl.nodes; p.st_ts_off = sl.frames; p.st_max_frames = st->max_frames; p.frames_done = st->frames_done;
  }
  hipStream_t s = (hipStream_t)a.stream;
  const bool fast_lm = lm && lm->d_ngs && lm->order - 1 <= kParCtx;
  const bool hom = lm && lm->homs.size() > 1;      // (a transcription model without a shared key takes the instances it always took)
  const int lmk = lmk_of(lm != nullptr, fast_lm, a.restricted, hom);
  if (!plan.general) {
    const void* fn = kernel_of(a.dtype, false, lmk, st != nullptr);
    E2E_HIP_CHECK(allow_dynamic_lds(fn, (int)l.lds), "hipFuncSetAttribute");
    void* args[] = { &p };
    E2E_HIP_CHECK(hipLaunchKernel(fn, dim3(a.B), dim3(kThreads), args, l.lds, s), "ctc_beam_kernel launch");
    E2E_HIP_CHECK(hipGetLastError(), "ctc_beam_kernel launch");
    return E2E_OK;
  }
  const GenLayout& gl = plan.g;
  GenParams g;
  g.gkey = reinterpret_cast<unsigned long long*>(ws + plan.gen_at + gl.gkey);
  g.lmc = lm ? reinterpret_cast<LmAnswer*>(ws + plan.gen_at + gl.lmc) : nullptr;
  g.gmem = gl.members_in_ws ? reinterpret_cast<unsigned char*>(ws + plan.gen_at + gl.gmem) : nullptr;
  g.CH = gl.CH;
  g.gstride = gl.gstride;
  g.cut_ids = nullptr; g.cut_n = nullptr; g.cut_k1 = 0;
  if (cut) {
    // the frames' label lists first, on the same stream: the search reads them
    int* const ids = reinterpret_cast<int*>(ws + plan.lists_at + plan.c.ids);
    int* const cn = reinterpret_cast<int*>(ws + plan.lists_at + plan.c.n);
    if (const int rc = launch_label_cut(a.lp, a.dtype, a.sB, a.sT, a.sV, a.x_len, a.B, a.T, a.V, a.blank, cut->top_n, cut->prob, ids, cn, s)) return rc;
    g.cut_ids = ids; g.cut_n = cn; g.cut_k1 = plan.c.K1;
  }
  const void* gfn = kernel_of(a.dtype, true, lmk, st != nullptr, cut != nullptr);
  E2E_HIP_CHECK(allow_dynamic_lds(gfn, (int)gl.lds), "hipFuncSetAttribute");
  void* gargs[] = { &p, &g };
  E2E_HIP_CHECK(hipLaunchKernel(gfn, dim3(a.B), dim3(kThreads), gargs, gl.lds, s), "ctc_beam_general_kernel launch");
  E2E_HIP_CHECK(hipGetLastError(), "ctc_beam_general_kernel launch");
  return E2E_OK;
}

extern "C" {

int e2e_ctc_beam(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len, int B, int T, int V, int blank,
                 int beam_width, int space_id, const e2e_lm* lm, double lmwt, double wip, double oov_penalty,
                 int64_t* out, int64_t max_out, int64_t* out_len, void* workspace, size_t workspace_bytes, void* stream) {
  const BeamArgs a = { lp, dtype, sB, sT, sV, x_len, B, T, V, blank, beam_width, space_id, lm, lmwt, wip, oov_penalty, false,
                       out, max_out, out_len, workspace, workspace_bytes, stream };
  return beam_run(a);
}

int e2e_ctc_beam_nbest(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len, int B, int T, int V,
                       int blank, int beam_width, int space_id, const e2e_lm* lm, double lmwt, double wip, double oov_penalty,
                       int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp, double* scores, int32_t* counts,
                       int64_t* timesteps, void* workspace, size_t workspace_bytes, void* stream) {
  const BeamArgs a = { lp, dtype, sB, sT, sV, x_len, B, T, V, blank, beam_width, space_id, lm, lmwt, wip, oov_penalty, false,
                       out, max_out, out_len, workspace, workspace_bytes, stream };
  const NBestOut nb = { nbest, n_hyp, scores, counts, timesteps };
  return beam_run(a, &nb);
}

int e2e_ctc_beam_nbest_opt(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len, int B, int T, int V,
                           int blank, int beam_width, int space_id, const e2e_lm* lm, double lmwt, double wip, double oov_penalty,
                           int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp, double* scores, int32_t* counts,
                           int64_t* timesteps, void* workspace, size_t workspace_bytes, void* stream, const e2e_ctc_beam_opts* opts) {
  const BeamArgs a = { lp, dtype, sB, sT, sV, x_len, B, T, V, blank, beam_width, space_id, lm, lmwt, wip, oov_penalty,
                       restricted_by(opts), out, max_out, out_len, workspace, workspace_bytes, stream };
  const NBestOut nb = { nbest, n_hyp, scores, counts, timesteps };
  return beam_run(a, &nb);
}

int e2e_ctc_beam_nbest_cut(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len, int B, int T, int V,
                           int blank, int beam_width, int space_id, const e2e_lm* lm, double lmwt, double wip, double oov_penalty,
                           int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp, double* scores, int32_t* counts,
                           int64_t* timesteps, void* workspace, size_t workspace_bytes, void* stream, const e2e_ctc_beam_opts* opts,
                           int cutoff_top_n, double cutoff_prob) {
  const BeamArgs a = { lp, dtype, sB, sT, sV, x_len, B, T, V, blank, beam_width, space_id, lm, lmwt, wip, oov_penalty,
                       restricted_by(opts), out, max_out, out_len, workspace, workspace_bytes, stream };
  const NBestOut nb = { nbest, n_hyp, scores, counts, timesteps };
  const CutIn cut = { cutoff_top_n, cutoff_prob };
  return beam_run(a, &nb, nullptr, &cut);
}

int e2e_ctc_beam_stream(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* chunk_len, int B, int T, int V,
                        int blank, int beam_width, int space_id, const e2e_lm* lm, double lmwt, double wip, double oov_penalty,
                        void* state, size_t row_bytes, int max_frames, int with_timesteps,
                        int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp, double* scores, int32_t* counts,
                        int64_t* timesteps, int64_t* frames_done, void* workspace, size_t workspace_bytes, void* stream,
                        const e2e_ctc_beam_opts* opts) {
  const BeamArgs a = { lp, dtype, sB, sT, sV, chunk_len, B, T, V, blank, beam_width, space_id, lm, lmwt, wip, oov_penalty,
                       restricted_by(opts), out, max_out, out_len, workspace, workspace_bytes, stream };
  const NBestOut nb = { nbest, n_hyp, scores, counts, timesteps };
  const StreamIn st = { state, row_bytes, max_frames, with_timesteps, frames_done };
  return beam_run(a, &nb, &st);
}

int e2e_ctc_beam_stream_cut(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* chunk_len, int B, int T, int V,
                            int blank, int beam_width, int space_id, const e2e_lm* lm, double lmwt, double wip, double oov_penalty,
                            void* state, size_t row_bytes, int max_frames, int with_timesteps,
                            int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp, double* scores, int32_t* counts,
                            int64_t* timesteps, int64_t* frames_done, void* workspace, size_t workspace_bytes, void* stream,
                            const e2e_ctc_beam_opts* opts, int cutoff_top_n, double cutoff_prob) {
  const BeamArgs a = { lp, dtype, sB, sT, sV, chunk_len, B, T, V, blank, beam_width, space_id, lm, lmwt, wip, oov_penalty,
                       restricted_by(opts), out, max_out, out_len, workspace, workspace_bytes, stream };
  const NBestOut nb = { nbest, n_hyp, scores, counts, timesteps };
  const StreamIn st = { state, row_bytes, max_frames, with_timesteps, frames_done };
  const CutIn cut = { cutoff_top_n, cutoff_prob };
  return beam_run(a, &nb, &st, &cut);
}

}  // extern "C"
