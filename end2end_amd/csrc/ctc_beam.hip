// Prefix beam search with optional n-gram LM scoring: the host side.  The algorithm, the types and the phases the kernels share
// are in ctc_beam_common.h, the kernels in ctc_beam_lds.hip (the beam in LDS) and ctc_beam_general.hip (any alphabet width), one
// object per input dtype each.  Here: the workspace and LDS layouts, which kernel a call takes (beam_fits / gen_fits /
// beam_takes_general), which of its instances (lmk_of, kernel_of), and the C entry points of include/e2e_ctc.h.
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
    default:      return kernel_of_io<bf16_t>(general, lmk, st, cut);     // (beam_call has checked the dtype)
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

// which kernel a call takes (same decision in the workspace query and in the call)
static bool beam_takes_general(int V, int W, bool lm) {
  static const bool force_general = getenv("E2E_BEAM_GENERAL") != nullptr;      // (tests: the whole suite through the general kernel)
  const bool fast_ok = beam_fits(V, W, lm), gen_ok = gen_fits(V, W, lm);
  return gen_ok && (!fast_ok || force_general);
}

extern "C" size_t e2e_ctc_beam_workspace_bytes_lm(int B, int T, int V, int beam_width, int with_lm) {
  if (B < 0 || T < 1 || V < 1 || beam_width < 1) return 0;
  const BeamLayout l = beam_layout(B, T, V, beam_width, with_lm != 0);
  // the general kernel's share (candidate keys, the LM's answer rows, member sets of very wide beams) only when that kernel
  // will run, its LM rows only with a language model: 6.4 MB per utterance instead of 19 at V = 8000, W = 100 without one
  const size_t gen = beam_takes_general(V, beam_width, with_lm != 0)
                         ? gen_layout(B, V, beam_width, l.WP2, l.HS, with_lm != 0).total : 0;
  return l.total + gen + 256;
}
// (sized for a call with a language model, which every call without one fits as well)
extern "C" size_t e2e_ctc_beam_workspace_bytes(int B, int T, int V, int beam_width) {
  const size_t a = e2e_ctc_beam_workspace_bytes_lm(B, T, V, beam_width, 1), b = e2e_ctc_beam_workspace_bytes_lm(B, T, V, beam_width, 0);
  return a > b ? a : b;
}

// the frames of the nodes, one int per node beside the node pool (e2e_ctc_beam_nbest with timestamps)
static size_t node_frames_bytes(int B, int NCAP) { return align_up((size_t)B * NCAP * sizeof(int), 256); }

// ---- a pruned call (e2e_ctc_beam_nbest_cut / e2e_ctc_beam_stream_cut) ----
// what it adds to the arguments of the unpruned call (null: not pruned), and the frames' label lists in its workspace:
// ids (B,T,K+1) then the counts (B,T), each 256-aligned, written by the selection kernel ahead of the search on the stream
struct CutIn { int top_n; double prob; };
struct CutLists { size_t ids, n, total; int K1; };
static CutLists cut_lists(int B, int T, int V, int top_n) {
  CutLists c;
  c.K1 = label_cut_k(V, top_n) + 1;
  c.ids = 0; c.n = align_up((size_t)B * T * c.K1 * sizeof(int), 256);
  c.total = c.n + align_up((size_t)B * T * sizeof(int), 256);
  return c;
}
static bool cut_prunes(int V, int top_n, double prob) { return top_n < V || prob < 1.0; }

extern "C" int e2e_ctc_beam_cut_max_width(int V, int with_lm) {
  if (V < 1) return 0;
  int lo = 0, hi = kGenMaxW;                    // (a pruned call always takes the general kernel)
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (gen_fits(V, mid, with_lm != 0)) lo = mid; else hi = mid - 1;
  }
  return lo;
}

extern "C" size_t e2e_ctc_beam_cut_workspace_bytes(int B, int T, int V, int beam_width, int with_lm, int with_timesteps,
                                                   int cutoff_top_n) {
  if (B < 0 || T < 1 || V < 1 || beam_width < 1 || cutoff_top_n < 1) return 0;
  const BeamLayout l = beam_layout(B, T, V, beam_width, with_lm != 0);
  const CutLists c = cut_lists(B, T, V, cutoff_top_n);
  const size_t pruned = l.total + gen_layout(B, V, beam_width, l.WP2, l.HS, with_lm != 0, c.K1).total +
                        (with_timesteps ? node_frames_bytes(B, l.NCAP) : 0) + c.total + 256;
  // (cutoff_top_n >= V prunes only with cutoff_prob < 1, which the query does not know: such a call may be the unpruned one)
  const size_t plain = cutoff_top_n >= V ? e2e_ctc_beam_nbest_workspace_bytes(B, T, V, beam_width, with_lm, with_timesteps) : 0;
  return pruned > plain ? pruned : plain;
}

extern "C" size_t e2e_ctc_beam_cut_stream_workspace_bytes(int B, int T, int V, int beam_width, int with_lm, int cutoff_top_n) {
  if (B < 0 || T < 1 || V < 1 || beam_width < 1 || cutoff_top_n < 1) return 0;
  const BeamLayout l = beam_layout(B, 1, V, beam_width, with_lm != 0);
  const size_t pruned = gen_layout(B, V, beam_width, l.WP2, l.HS, with_lm != 0, cut_lists(B, T, V, cutoff_top_n).K1).total +
                        cut_lists(B, T, V, cutoff_top_n).total + 256;
  const size_t plain = cutoff_top_n >= V ? e2e_ctc_beam_stream_workspace_bytes(B, V, beam_width, with_lm) : 0;
  return pruned > plain ? pruned : plain;
}

extern "C" size_t e2e_ctc_beam_nbest_workspace_bytes(int B, int T, int V, int beam_width, int with_lm, int with_timesteps) {
  const size_t base = e2e_ctc_beam_workspace_bytes_lm(B, T, V, beam_width, with_lm);
  if (!base || !with_timesteps) return base;
  return base + node_frames_bytes(B, beam_layout(B, T, V, beam_width, with_lm != 0).NCAP);
}

// what e2e_ctc_beam_nbest adds to the arguments of e2e_ctc_beam (null: the plain call)
struct NBestOut { int nbest; int64_t* n_hyp; double* scores; int32_t* counts; int64_t* timesteps; };

// ... and e2e_ctc_beam_stream (null: a call that decodes whole utterances)
struct StreamIn { void* state; size_t row_bytes; int max_frames, with_timesteps; int64_t* frames_done; };
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

extern "C" size_t e2e_ctc_beam_stream_workspace_bytes(int B, int V, int beam_width, int with_lm) {
  if (B < 0 || V < 1 || beam_width < 1) return 0;
  if (!beam_takes_general(V, beam_width, with_lm != 0)) return 0;
  const BeamLayout l = beam_layout(B, 1, V, beam_width, with_lm != 0);
  return gen_layout(B, V, beam_width, l.WP2, l.HS, with_lm != 0).total + 256;
}

static int beam_call(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV,
                     const int64_t* x_len, int B, int T, int V, int blank,
                     int beam_width, int space_id, const e2e_lm* lm,
                     double lmwt, double wip, double oov_penalty,
                     int64_t* out, int64_t max_out, int64_t* out_len, const NBestOut* nb, bool restricted,
                     void* workspace, size_t workspace_bytes, void* stream, const StreamIn* st = nullptr,
                     const CutIn* cut = nullptr) {
  if (dtype != E2E_F32 && dtype != E2E_F64 && !dtype_is_16bit(dtype)) { set_error("dtype must be E2E_F32, E2E_F64, E2E_F16 or E2E_BF16"); return E2E_ERR_ARG; }
  if (B < 0 || T < 1 || V < 1 || beam_width < 1 || max_out < 1) { set_error("bad sizes"); return E2E_ERR_ARG; }
  if (blank < 0 || blank >= V) { set_error("blank=%d outside [0,%d)", blank, V); return E2E_ERR_ARG; }
  if (B > 0 && (!lp || !x_len || ((!out || !out_len) && !(st && nb->nbest == 0)))) { set_error("null pointer argument"); return E2E_ERR_ARG; }
  if (const int rc = check_model_device(lm)) return rc;
  // the kernel spells words with label_off[0..V]: the model must have been loaded with exactly this alphabet
  if (lm && (int)lm->label_off.size() - 1 != V) {
    set_error("the language model was loaded with %d labels but the log-probabilities have %d columns",
              (int)lm->label_off.size() - 1, V);
    return E2E_ERR_ARG;
  }
  // (a stream: the node pool is the row's, sized by max_frames; the workspace holds the general kernel's share alone)
  const BeamLayout l = beam_layout(B, st ? st->max_frames : T, V, beam_width, lm != nullptr);
  const bool fast_ok = beam_fits(V, beam_width, lm != nullptr), gen_ok = gen_fits(V, beam_width, lm != nullptr);
  const bool general = cut ? true : beam_takes_general(V, beam_width, lm != nullptr);
  if (cut) if (const int rc = label_cut_check(dtype, B, T, V, blank, cut->top_n, cut->prob)) return rc;
  if (cut ? !gen_ok : !fast_ok && !gen_ok) {
    set_error("beam_width = %d over an alphabet of %d%s: at most %d (one workgroup's LDS holds the beam)", beam_width, V,
              lm ? " with a language model" : "", cut ? e2e_ctc_beam_cut_max_width(V, lm != nullptr) : e2e_ctc_beam_max_width(V, lm != nullptr));
    return E2E_ERR_UNSUPPORTED;
  }
  CutLists cl; cl.ids = cl.n = cl.total = 0; cl.K1 = 0;
  if (cut) cl = cut_lists(B, T, V, cut->top_n);
  const GenLayout gl = gen_layout(B, V, beam_width, l.WP2, l.HS, lm != nullptr, cl.K1);
  uintptr_t base = reinterpret_cast<uintptr_t>(workspace);
  const uintptr_t aligned = (base + 255) & ~(uintptr_t)255;
  const size_t gen_at = st ? 0 : l.total;
  const size_t frames_at = gen_at + (general ? gl.total : 0);
  const size_t lists_at = frames_at + (!st && nb && nb->timesteps ? node_frames_bytes(B, l.NCAP) : 0);
  const size_t need = lists_at + cl.total;
  if (need && (!workspace || workspace_bytes < need + (aligned - base))) { set_error("workspace too small: need %zu", need + 256); return E2E_ERR_WORKSPACE; }
  if (B == 0) return E2E_OK;
  char* ws = reinterpret_cast<char*>(aligned);
  BeamParams p;
  p.lp = lp; p.sB = sB; p.sT = sT; p.sV = sV; p.x_len = x_len;
  p.B = B; p.T = T; p.V = V; p.blank = blank; p.W = beam_width; p.space_id = space_id;
  p.has_lm = lm ? 1 : 0;
  if (lm) p.lm = lm->dev_view(); else memset(&p.lm, 0, sizeof(p.lm));
  p.lmwt = lm ? lmwt : 0.0;                       // ctc_decoder.cpp:72-74
  p.wip = wip; p.oov = oov_penalty;
  p.out = out; p.max_out = max_out; p.out_len = out_len;
  p.nodes = reinterpret_cast<BeamNode*>(ws + l.nodes);
  p.NCAP = l.NCAP; p.CMAX = l.CMAX; p.WP2 = l.WP2; p.HS = l.HS;
  p.nbest = nb ? nb->nbest : 0;
  p.n_hyp = nb ? nb->n_hyp : nullptr; p.scores = nb ? nb->scores : nullptr; p.counts = nb ? nb->counts : nullptr;
  p.ts_out = nb ? nb->timesteps : nullptr;
  p.node_t = !st && nb && nb->timesteps ? reinterpret_cast<int*>(ws + frames_at) : nullptr;
  p.st_rows = nullptr; p.st_row_bytes = 0; p.st_nodes_off = 0; p.st_ts_off = 0; p.st_max_frames = 0; p.frames_done = nullptr;
  if (st) {
    const StreamLayout sl = stream_layout(st->max_frames, V, beam_width, lm != nullptr, st->with_timesteps != 0);
    p.nodes = nullptr;
    p.st_rows = static_cast<unsigned char*>(st->state); p.st_row_bytes = st->row_bytes;
    p.st_nodes_off = sl.nodes; p.st_ts_off = sl.frames; p.st_max_frames = st->max_frames; p.frames_done = st->frames_done;
  }
  hipStream_t s = (hipStream_t)stream;
  const bool fast_lm = lm && lm->d_ngs && lm->order - 1 <= kParCtx;
  const bool hom = lm && lm->homs.size() > 1;      // (a transcription model without a shared key takes the instances it always took)
  const int lmk = lmk_of(lm != nullptr, fast_lm, restricted, hom);
  if (general) {
    GenParams g;
    g.gkey = reinterpret_cast<unsigned long long*>(ws + gen_at + gl.gkey);
    g.lmc = lm ? reinterpret_cast<LmAnswer*>(ws + gen_at + gl.lmc) : nullptr;
    g.gmem = gl.members_in_ws ? reinterpret_cast<unsigned char*>(ws + gen_at + gl.gmem) : nullptr;
    g.CH = gl.CH;
    g.gstride = gl.gstride;
    g.cut_ids = nullptr; g.cut_n = nullptr; g.cut_k1 = 0;
    if (cut) {
      // the frames' label lists first, on the same stream: the search reads them
      int* const ids = reinterpret_cast<int*>(ws + lists_at + cl.ids);
      int* const cn = reinterpret_cast<int*>(ws + lists_at + cl.n);
      if (const int rc = launch_label_cut(lp, dtype, sB, sT, sV, x_len, B, T, V, blank, cut->top_n, cut->prob, ids, cn, s)) return rc;
      g.cut_ids = ids; g.cut_n = cn; g.cut_k1 = cl.K1;
    }
    const void* gfn = kernel_of(dtype, true, lmk, st != nullptr, cut != nullptr);
    E2E_HIP_CHECK(allow_dynamic_lds(gfn, (int)gl.lds), "hipFuncSetAttribute");
    void* gargs[] = { &p, &g };
    E2E_HIP_CHECK(hipLaunchKernel(gfn, dim3(B), dim3(kThreads), gargs, gl.lds, s), "ctc_beam_general_kernel launch");
    E2E_HIP_CHECK(hipGetLastError(), "ctc_beam_general_kernel launch");
    return E2E_OK;
  }
  const void* fn = kernel_of(dtype, false, lmk, st != nullptr);
  E2E_HIP_CHECK(allow_dynamic_lds(fn, (int)l.lds), "hipFuncSetAttribute");
  void* args[] = { &p };
  E2E_HIP_CHECK(hipLaunchKernel(fn, dim3(B), dim3(kThreads), args, l.lds, s), "ctc_beam_kernel launch");
  E2E_HIP_CHECK(hipGetLastError(), "ctc_beam_kernel launch");
  return E2E_OK;
}

extern "C" int e2e_ctc_beam(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV,
                            const int64_t* x_len, int B, int T, int V, int blank,
                            int beam_width, int space_id, const e2e_lm* lm,
                            double lmwt, double wip, double oov_penalty,
                            int64_t* out, int64_t max_out, int64_t* out_len,
                            void* workspace, size_t workspace_bytes, void* stream) {
  return beam_call(lp, dtype, sB, sT, sV, x_len, B, T, V, blank, beam_width, space_id, lm, lmwt, wip, oov_penalty,
                   out, max_out, out_len, nullptr, false, workspace, workspace_bytes, stream);
}

static int nbest_call(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV,
                      const int64_t* x_len, int B, int T, int V, int blank,
                      int beam_width, int space_id, const e2e_lm* lm,
                      double lmwt, double wip, double oov_penalty,
                      int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp,
                      double* scores, int32_t* counts, int64_t* timesteps, bool restricted,
                      void* workspace, size_t workspace_bytes, void* stream, const CutIn* cut = nullptr) {
  if (beam_width < 1 || nbest < 1 || nbest > beam_width) { set_error("nbest=%d outside [1, beam_width=%d]", nbest, beam_width); return E2E_ERR_ARG; }
  if (B > 0 && (!n_hyp || !scores || !counts || !out || !out_len)) { set_error("null pointer argument"); return E2E_ERR_ARG; }
  const int cap = V < 1 ? 0 : cut ? e2e_ctc_beam_cut_max_width(V, lm != nullptr) : e2e_ctc_beam_max_width(V, lm != nullptr);
  if (V >= 1 && beam_width > cap) {
    set_error("beam_width = %d over an alphabet of %d%s: at most %d", beam_width, V, lm ? " with a language model" : "", cap);
    return E2E_ERR_ARG;
  }
  const NBestOut nb = { nbest, n_hyp, scores, counts, timesteps };
  return beam_call(lp, dtype, sB, sT, sV, x_len, B, T, V, blank, beam_width, space_id, lm, lmwt, wip, oov_penalty,
                   out, max_out, out_len, &nb, restricted, workspace, workspace_bytes, stream, nullptr, cut);
}

extern "C" int e2e_ctc_beam_nbest(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV,
                                  const int64_t* x_len, int B, int T, int V, int blank,
                                  int beam_width, int space_id, const e2e_lm* lm,
                                  double lmwt, double wip, double oov_penalty,
                                  int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp,
                                  double* scores, int32_t* counts, int64_t* timesteps,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  return nbest_call(lp, dtype, sB, sT, sV, x_len, B, T, V, blank, beam_width, space_id, lm, lmwt, wip, oov_penalty,
                    nbest, out, max_out, out_len, n_hyp, scores, counts, timesteps, false, workspace, workspace_bytes, stream);
}

static int nbest_opt_call(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV,
                          const int64_t* x_len, int B, int T, int V, int blank,
                          int beam_width, int space_id, const e2e_lm* lm,
                          double lmwt, double wip, double oov_penalty,
                          int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp,
                          double* scores, int32_t* counts, int64_t* timesteps,
                          void* workspace, size_t workspace_bytes, void* stream, const e2e_ctc_beam_opts* opts, const CutIn* cut) {
  const bool restricted = opts && opts->restrict_to_lexicon != 0;
  if (restricted && (!lm || !lm->has_lexicon)) {
    set_error(lm ? "restrict_to_lexicon: the model has no lexicon (e2e_lm_enable_lexicon)" : "restrict_to_lexicon needs a model: a language model or a word list (e2e_lm_load_words)");
    return E2E_ERR_ARG;
  }
  return nbest_call(lp, dtype, sB, sT, sV, x_len, B, T, V, blank, beam_width, space_id, lm, lmwt, wip, oov_penalty,
                    nbest, out, max_out, out_len, n_hyp, scores, counts, timesteps, restricted, workspace, workspace_bytes, stream, cut);
}

extern "C" int e2e_ctc_beam_nbest_opt(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV,
                                      const int64_t* x_len, int B, int T, int V, int blank,
                                      int beam_width, int space_id, const e2e_lm* lm,
                                      double lmwt, double wip, double oov_penalty,
                                      int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp,
                                      double* scores, int32_t* counts, int64_t* timesteps,
                                      void* workspace, size_t workspace_bytes, void* stream, const e2e_ctc_beam_opts* opts) {
  return nbest_opt_call(lp, dtype, sB, sT, sV, x_len, B, T, V, blank, beam_width, space_id, lm, lmwt, wip, oov_penalty,
                        nbest, out, max_out, out_len, n_hyp, scores, counts, timesteps, workspace, workspace_bytes, stream, opts, nullptr);
}

// the cut's own argument errors, for the calls that forward to the unpruned ones when nothing is pruned
static int cut_args(int cutoff_top_n, double cutoff_prob) {
  if (cutoff_top_n < 1) { set_error("cutoff_top_n=%d: at least 1", cutoff_top_n); return E2E_ERR_ARG; }
  if (!(cutoff_prob > 0.0 && cutoff_prob <= 1.0)) { set_error("cutoff_prob=%g outside (0, 1]", cutoff_prob); return E2E_ERR_ARG; }
  return E2E_OK;
}

extern "C" int e2e_ctc_beam_nbest_cut(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV,
                                      const int64_t* x_len, int B, int T, int V, int blank,
                                      int beam_width, int space_id, const e2e_lm* lm,
                                      double lmwt, double wip, double oov_penalty,
                                      int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp,
                                      double* scores, int32_t* counts, int64_t* timesteps,
                                      void* workspace, size_t workspace_bytes, void* stream, const e2e_ctc_beam_opts* opts,
                                      int cutoff_top_n, double cutoff_prob) {
  if (const int rc = cut_args(cutoff_top_n, cutoff_prob)) return rc;
  const CutIn cut = { cutoff_top_n, cutoff_prob };
  return nbest_opt_call(lp, dtype, sB, sT, sV, x_len, B, T, V, blank, beam_width, space_id, lm, lmwt, wip, oov_penalty,
                        nbest, out, max_out, out_len, n_hyp, scores, counts, timesteps, workspace, workspace_bytes, stream, opts,
                        cut_prunes(V, cutoff_top_n, cutoff_prob) ? &cut : nullptr);
}

static int stream_call(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV,
                       const int64_t* chunk_len, int B, int T, int V, int blank,
                       int beam_width, int space_id, const e2e_lm* lm,
                       double lmwt, double wip, double oov_penalty,
                       void* state, size_t row_bytes, int max_frames, int with_timesteps,
                       int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp,
                       double* scores, int32_t* counts, int64_t* timesteps, int64_t* frames_done,
                       void* workspace, size_t workspace_bytes, void* stream, const e2e_ctc_beam_opts* opts, const CutIn* cut) {
  // every argument error the host can see, before any launch
  if (B < 0 || T < 1 || V < 1 || beam_width < 1 || max_frames < 1) { set_error("bad sizes"); return E2E_ERR_ARG; }
  if (nbest < 0 || nbest > beam_width) { set_error("nbest=%d outside [0, beam_width=%d]", nbest, beam_width); return E2E_ERR_ARG; }
  if (B > 0 && (!state || !frames_done || !chunk_len)) { set_error("null pointer argument"); return E2E_ERR_ARG; }
  if (B > 0 && nbest > 0 && (!n_hyp || !scores || !counts || !out || !out_len)) { set_error("null pointer argument"); return E2E_ERR_ARG; }
  if (!with_timesteps && timesteps) { set_error("timesteps asked of a stream that was opened with_timesteps = 0"); return E2E_ERR_ARG; }
  const int cap = cut ? e2e_ctc_beam_cut_max_width(V, lm != nullptr) : e2e_ctc_beam_max_width(V, lm != nullptr);
  if (beam_width > cap) {
    set_error("beam_width = %d over an alphabet of %d%s: at most %d", beam_width, V, lm ? " with a language model" : "", cap);
    return E2E_ERR_ARG;
  }
  const size_t want = e2e_ctc_beam_stream_row_bytes(max_frames, V, beam_width, lm != nullptr, with_timesteps);
  if (!want) { set_error("max_frames = %d: the node pool of a stream this long cannot be indexed", max_frames); return E2E_ERR_ARG; }
  if (row_bytes < want || row_bytes % 8) {
    set_error("row_bytes = %zu: a state row needs %zu bytes (e2e_ctc_beam_stream_row_bytes) and a multiple of 8", row_bytes, want);
    return E2E_ERR_ARG;
  }
  if (B > 0 && reinterpret_cast<uintptr_t>(state) % 8) { set_error("the state must be 8-byte aligned"); return E2E_ERR_ARG; }
  const bool restricted = opts && opts->restrict_to_lexicon != 0;
  if (restricted && (!lm || !lm->has_lexicon)) {
    set_error(lm ? "restrict_to_lexicon: the model has no lexicon (e2e_lm_enable_lexicon)" : "restrict_to_lexicon needs a model: a language model or a word list (e2e_lm_load_words)");
    return E2E_ERR_ARG;
  }
  const NBestOut nb = { nbest, n_hyp, scores, counts, nbest > 0 ? timesteps : nullptr };
  const StreamIn st = { state, row_bytes, max_frames, with_timesteps, frames_done };
  return beam_call(lp, dtype, sB, sT, sV, chunk_len, B, T, V, blank, beam_width, space_id, lm, lmwt, wip, oov_penalty,
                   out, nbest > 0 ? max_out : 1, out_len, &nb, restricted, workspace, workspace_bytes, stream, &st, cut);
}

extern "C" int e2e_ctc_beam_stream(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV,
                                   const int64_t* chunk_len, int B, int T, int V, int blank,
                                   int beam_width, int space_id, const e2e_lm* lm,
                                   double lmwt, double wip, double oov_penalty,
                                   void* state, size_t row_bytes, int max_frames, int with_timesteps,
                                   int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp,
                                   double* scores, int32_t* counts, int64_t* timesteps, int64_t* frames_done,
                                   void* workspace, size_t workspace_bytes, void* stream, const e2e_ctc_beam_opts* opts) {
  return stream_call(lp, dtype, sB, sT, sV, chunk_len, B, T, V, blank, beam_width, space_id, lm, lmwt, wip, oov_penalty,
                     state, row_bytes, max_frames, with_timesteps, nbest, out, max_out, out_len, n_hyp, scores, counts, timesteps,
                     frames_done, workspace, workspace_bytes, stream, opts, nullptr);
}

extern "C" int e2e_ctc_beam_stream_cut(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV,
                                       const int64_t* chunk_len, int B, int T, int V, int blank,
                                       int beam_width, int space_id, const e2e_lm* lm,
                                       double lmwt, double wip, double oov_penalty,
                                       void* state, size_t row_bytes, int max_frames, int with_timesteps,
                                       int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp,
                                       double* scores, int32_t* counts, int64_t* timesteps, int64_t* frames_done,
                                       void* workspace, size_t workspace_bytes, void* stream, const e2e_ctc_beam_opts* opts,
                                       int cutoff_top_n, double cutoff_prob) {
  if (const int rc = cut_args(cutoff_top_n, cutoff_prob)) return rc;
  const CutIn cut = { cutoff_top_n, cutoff_prob };
  return stream_call(lp, dtype, sB, sT, sV, chunk_len, B, T, V, blank, beam_width, space_id, lm, lmwt, wip, oov_penalty,
                     state, row_bytes, max_frames, with_timesteps, nbest, out, max_out, out_len, n_hyp, scores, counts, timesteps,
                     frames_done, workspace, workspace_bytes, stream, opts, cut_prunes(V, cutoff_top_n, cutoff_prob) ? &cut : nullptr);
}

