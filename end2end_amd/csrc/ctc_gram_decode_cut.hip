// Gram-CTC beam search with per-frame label pruning (cutoff_top_n, cutoff_prob): e2e_gram_ctc_beam_nbest_cut and
// e2e_gram_ctc_beam_stream_cut.  The definition is in include/e2e_ctc.h beside e2e_gram_ctc_beam_nbest, the account in
// DESIGN.md 4.7, Pruned.
//
// A call is two kernels on the caller's stream: the selection (launch_label_cut, ctc_label_cut.hip; blank 0) writes every
// frame's kept columns, ascending and the blank first, into the head of the workspace, and the CUT instance of
// gram_beam_kernel (ctc_gram_decode.h) expands those alone.  The eight CUT instances live in this object so that they
// build beside the unpruned ones; they share one parameter block (GramCutParams).  Nothing of a frame's work scales with V:
// the pair space is W * (K + 1), K = min(cutoff_top_n, V), which is also what the width limit and the workspace are made of,
// and there is no answer cache.
#include "ctc_gram_decode.h"

namespace e2e {
namespace beamk {
// (ctc_label_cut.hip; declared in ctc_beam_common.h, which is the CTC search's device code)
int label_cut_check(int dtype, int B, int T, int V, int blank, int cutoff_top_n, double cutoff_prob);
int launch_label_cut(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len, int B, int T, int V,
                     int blank, int cutoff_top_n, double cutoff_prob, int* ids, int* n, hipStream_t s);
}  // namespace beamk

namespace {

// K + 1: the stride of a frame's list and of a member's pairs
int cut_stride(int V, int top_n) { return (top_n < V ? top_n : V) + 1; }
bool cut_prunes(int V, int top_n, double prob) { return top_n < V || prob < 1.0; }

// the head of the workspace: ids (B,T,S) and cnt (B,T) int32, each 256-aligned; behind them the utterances' search buffers
struct CutLists { size_t off_cnt, bytes; };
CutLists cut_lists(int B, int T, int S) {
  CutLists c;
  c.off_cnt = align_up((size_t)B * T * S * 4, 256);
  c.bytes = c.off_cnt + align_up((size_t)B * T * 4, 256);
  return c;
}

// what the host can see of the knobs, before any launch; prunes: false for a call that is the unpruned one
int check_cut_knobs(int V, int top_n, double prob, bool& prunes) {
  if (top_n < 1) { set_error("cutoff_top_n=%d: at least 1", top_n); return E2E_ERR_ARG; }
  if (!(prob > 0.0 && prob <= 1.0)) { set_error("cutoff_prob=%g outside (0, 1]", prob); return E2E_ERR_ARG; }
  prunes = cut_prunes(V, top_n, prob);
  return E2E_OK;
}

// can a pruned call of these sizes run at all (the queries return 0 where it cannot)
bool cut_supported(int B, int T, int V, int max_order, int beam_width, int top_n) {
  return B >= 0 && T >= 1 && V >= 1 && top_n >= 1 && beam_width >= 1 && (int64_t)B * T <= 0x7fffffffLL / 2 &&
         cut_stride(V, top_n) - 1 <= e2e_ctc_label_cut_max() && beam_width <= e2e_gram_beam_cut_max_width(V, max_order, top_n);
}

int launch_cut_lists(GramCutParams& c, const GramBeamParams& p, void* workspace, const CutLists& cl, int S, int top_n, double prob,
                     hipStream_t s) {
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  int* ids = reinterpret_cast<int*>(w);
  int* cnt = reinterpret_cast<int*>(w + cl.off_cnt);
  c.ids = ids; c.cnt = cnt; c.S = S;
  return beamk::launch_label_cut(p.lp, p.dtype, p.sB, p.sT, p.sV, p.x_len, p.B, p.T, p.V, 0, top_n, prob, ids, cnt, s);
}

}  // namespace
}  // namespace e2e

using namespace e2e;

extern "C" {

int e2e_gram_beam_cut_max_width(int V, int max_order, int cutoff_top_n) {
  if (V < 1 || max_order < 1 || max_order > kMaxK || cutoff_top_n < 1) return 0;
  const int w = kMaxPairs / cut_stride(V, cutoff_top_n);
  return w < kMaxW ? w : kMaxW;
}

// (cutoff_top_n >= V prunes only with cutoff_prob < 1, which the queries do not know: such a call may be the unpruned one)
size_t e2e_gram_beam_cut_workspace_bytes(int B, int T, int V, int max_order, int beam_width, int scored, int with_lm, int cutoff_top_n) {
  if (with_lm && !scored) return 0;
  size_t pruned = 0;
  BeamLayout L;
  if (cut_supported(B, T, V, max_order, beam_width, cutoff_top_n) && beam_layout(T, cut_stride(V, cutoff_top_n), max_order, beam_width, L))
    pruned = cut_lists(B, T, cut_stride(V, cutoff_top_n)).bytes + (size_t)B * L.per_utt + 256;
  const size_t plain = cutoff_top_n >= V ? e2e_gram_beam_workspace_bytes_lm(B, T, V, max_order, beam_width, with_lm) : 0;
  return pruned > plain ? pruned : plain;
}

size_t e2e_gram_beam_cut_stream_workspace_bytes(int B, int T, int V, int max_order, int beam_width, int scored, int with_lm,
                                                int cutoff_top_n) {
  if (with_lm && !scored) return 0;
  size_t pruned = 0;
  StreamLayout S; BeamLayout L;
  if (cut_supported(B, T, V, max_order, beam_width, cutoff_top_n) &&
      stream_layout(1, cut_stride(V, cutoff_top_n), max_order, beam_width, scored != 0, false, S, L))
    pruned = cut_lists(B, T, cut_stride(V, cutoff_top_n)).bytes + (size_t)B * S.ws_per_utt + 256;
  const size_t plain = cutoff_top_n >= V ? e2e_gram_beam_stream_workspace_bytes(B, V, max_order, beam_width, scored, with_lm) : 0;
  return pruned > plain ? pruned : plain;
}

size_t e2e_gram_beam_cut_stream_row_bytes(int max_frames, int V, int max_order, int beam_width, int scored, int with_lm,
                                          int cutoff_top_n) {
  if (V < 1 || cutoff_top_n < 1 || (with_lm && !scored)) return 0;
  if (cutoff_top_n >= V) {                                       // (may be the unpruned call: the row is the same where both run)
    const size_t plain = e2e_gram_beam_stream_row_bytes(max_frames, V, max_order, beam_width, scored, with_lm);
    if (plain) return plain;
  }
  if (cut_stride(V, cutoff_top_n) - 1 > e2e_ctc_label_cut_max()) return 0;
  StreamLayout S; BeamLayout L;
  return stream_layout(max_frames, cut_stride(V, cutoff_top_n), max_order, beam_width, scored != 0, false, S, L) ? S.total : 0;
}

int e2e_gram_ctc_beam_nbest_cut(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len,
                                int B, int T, int V, const int32_t* gram_ids, const int32_t* gram_len, int max_order,
                                int num_base_labels, int beam_width, int scored, int space_id, const e2e_lm* lm, double lmwt,
                                double wip, double oov_penalty, int nbest, int64_t* out, int64_t max_out, int64_t* out_len,
                                int64_t* n_hyp, double* scores, int32_t* counts, void* workspace, size_t workspace_bytes,
                                void* stream, const e2e_gram_beam_opts* opts, int cutoff_top_n, double cutoff_prob) {
  const bool sc = scored != 0;
  // every argument error the host can see, before any launch
  bool prunes = false;
  if (const int rc = check_cut_knobs(V, cutoff_top_n, cutoff_prob, prunes)) return rc;
  if (!sc && (lm || counts || opts)) {
    set_error("scored = 0 is the search of e2e_gram_ctc_beam_nbest: lm, counts and opts must be NULL");
    return E2E_ERR_ARG;
  }
  if (!prunes) {                                                 // no pruning: the unpruned entries, kernel and workspace
    if (!sc) return e2e_gram_ctc_beam_nbest(lp, dtype, sB, sT, sV, x_len, B, T, V, gram_ids, gram_len, max_order, beam_width, nbest,
                                            out, max_out, out_len, n_hyp, scores, workspace, workspace_bytes, stream);
    return e2e_gram_ctc_beam_nbest_opt(lp, dtype, sB, sT, sV, x_len, B, T, V, gram_ids, gram_len, max_order, num_base_labels,
                                       beam_width, space_id, lm, lmwt, wip, oov_penalty, nbest, out, max_out, out_len, n_hyp,
                                       scores, counts, workspace, workspace_bytes, stream, opts);
  }
  const bool restricted = sc && opts && opts->restrict_to_lexicon != 0;
  int64_t* timesteps = sc && opts ? opts->timesteps : nullptr;
  if (dtype != E2E_F32 && dtype != E2E_F64) { set_error("dtype must be E2E_F32 or E2E_F64"); return E2E_ERR_ARG; }
  if (const int rc = beamk::label_cut_check(dtype, B, T, V, 0, cutoff_top_n, cutoff_prob)) return rc;
  if (const int rc = check_beam_args(dtype, B, T, V, max_order, beam_width, nbest, max_out, 1, cutoff_top_n)) return rc;
  if (sc) { if (const int rc = check_scored_args(V, num_base_labels, space_id, lm, restricted)) return rc; }
  const int S = cut_stride(V, cutoff_top_n);
  BeamLayout L;
  if (!beam_layout(T, S, max_order, beam_width, L)) { set_error("T=%d frames are more than the search takes", T); return E2E_ERR_UNSUPPORTED; }
  if (const int rc = check_pointers(B, {lp, x_len, gram_ids, gram_len, out_len, n_hyp, scores, sc ? counts : unused,
                                        max_out > 0 ? out : unused})) return rc;
  if (B == 0) return E2E_OK;
  if (const int rc = check_model_device(lm)) return rc;
  const CutLists cl = cut_lists(B, T, S);
  if (const int rc = check_workspace(workspace, workspace_bytes, cl.bytes + (size_t)B * L.per_utt, "e2e_gram_beam_cut_workspace_bytes")) return rc;
  GramCutParams c;
  memset(&c, 0, sizeof(c));
  GramLmParams& q = c.sp.o.l;
  fill_params(q.b, lp, dtype, sB, sT, sV, x_len, B, T, V, gram_ids, gram_len, max_order, beam_width, nbest, out, max_out, out_len,
              n_hyp, scores, reinterpret_cast<unsigned char*>(workspace) + cl.bytes, L, L.per_utt, L.off_nodes);
  fill_lm_params(q, num_base_labels, space_id, lm, lmwt, wip, oov_penalty, counts, L);
  c.sp.o.timesteps = timesteps;
  hipStream_t s = (hipStream_t)stream;
  if (const int rc = launch_cut_lists(c, q.b, workspace, cl, S, cutoff_top_n, cutoff_prob, s)) return rc;
  const dim3 g(B), t(kBeamThreads);
  if (!sc) hipLaunchKernelGGL((gram_beam_kernel<false, false, false, false, true>), g, t, 0, s, c);
  else if (!restricted && !timesteps) hipLaunchKernelGGL((gram_beam_kernel<true, false, false, false, true>), g, t, 0, s, c);
  else if (!restricted) hipLaunchKernelGGL((gram_beam_kernel<true, false, true, false, true>), g, t, 0, s, c);
  else if (!timesteps) hipLaunchKernelGGL((gram_beam_kernel<true, true, false, false, true>), g, t, 0, s, c);
  else hipLaunchKernelGGL((gram_beam_kernel<true, true, true, false, true>), g, t, 0, s, c);
  E2E_HIP_CHECK(hipGetLastError(), "gram_beam_kernel (pruned) launch");
  return E2E_OK;
}

int e2e_gram_ctc_beam_stream_cut(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* chunk_len,
                                 int B, int T, int V, const int32_t* gram_ids, const int32_t* gram_len, int max_order,
                                 int num_base_labels, int beam_width, int scored, int space_id, const e2e_lm* lm, double lmwt,
                                 double wip, double oov_penalty, void* state, size_t row_bytes, int max_frames,
                                 int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp, double* scores,
                                 int32_t* counts, int64_t* frames_done, void* workspace, size_t workspace_bytes, void* stream,
                                 const e2e_gram_beam_opts* opts, int cutoff_top_n, double cutoff_prob) {
  const bool sc = scored != 0;
  bool prunes = false;
  if (const int rc = check_cut_knobs(V, cutoff_top_n, cutoff_prob, prunes)) return rc;
  if (!prunes)
    return e2e_gram_ctc_beam_stream(lp, dtype, sB, sT, sV, chunk_len, B, T, V, gram_ids, gram_len, max_order, num_base_labels,
                                    beam_width, scored, space_id, lm, lmwt, wip, oov_penalty, state, row_bytes, max_frames, nbest,
                                    out, max_out, out_len, n_hyp, scores, counts, frames_done, workspace, workspace_bytes, stream, opts);
  const bool restricted = sc && opts && opts->restrict_to_lexicon != 0;
  if (dtype != E2E_F32 && dtype != E2E_F64) { set_error("dtype must be E2E_F32 or E2E_F64"); return E2E_ERR_ARG; }
  if (const int rc = beamk::label_cut_check(dtype, B, T, V, 0, cutoff_top_n, cutoff_prob)) return rc;
  if (const int rc = check_beam_args(dtype, B, T, V, max_order, beam_width, nbest, nbest > 0 ? max_out : 0, 0, cutoff_top_n)) return rc;
  if (!sc && (lm || counts || opts)) {
    set_error("scored = 0 is the search of e2e_gram_ctc_beam_nbest: lm, counts and opts must be NULL");
    return E2E_ERR_ARG;
  }
  if (sc) { if (const int rc = check_scored_args(V, num_base_labels, space_id, lm, restricted)) return rc; }
  if (max_frames < 1 || max_frames > (1 << 22)) { set_error("max_frames=%d outside [1, %d]", max_frames, 1 << 22); return E2E_ERR_ARG; }
  const int S = cut_stride(V, cutoff_top_n);
  StreamLayout SL; BeamLayout L;
  if (!stream_layout(max_frames, S, max_order, beam_width, sc, false, SL, L)) {
    set_error("max_frames=%d frames are more than the search takes", max_frames); return E2E_ERR_UNSUPPORTED;
  }
  if (const int rc = check_row_bytes(row_bytes, SL.total, "e2e_gram_beam_cut_stream_row_bytes")) return rc;
  if (const int rc = check_pointers(B, {lp, chunk_len, gram_ids, gram_len, state, frames_done})) return rc;
  if (nbest > 0) if (const int rc = check_pointers(B, {out_len, n_hyp, scores, sc ? counts : unused, max_out > 0 ? out : unused})) return rc;
  if (const int rc = check_state_aligned(B, state)) return rc;
  if (B == 0) return E2E_OK;
  const CutLists cl = cut_lists(B, T, S);
  if (const int rc = check_workspace(workspace, workspace_bytes, cl.bytes + (size_t)B * SL.ws_per_utt, "e2e_gram_beam_cut_stream_workspace_bytes")) return rc;
  if (const int rc = check_model_device(lm)) return rc;
  GramCutParams c;
  memset(&c, 0, sizeof(c));
  GramLmParams& q = c.sp.o.l;
  fill_params(q.b, lp, dtype, sB, sT, sV, chunk_len, B, T, V, gram_ids, gram_len, max_order, beam_width, nbest, out,
              nbest > 0 ? max_out : 0, out_len, n_hyp, scores, reinterpret_cast<unsigned char*>(workspace) + cl.bytes, L,
              SL.ws_per_utt, 0);                                                                       // (the nodes are the row's)
  fill_lm_params(q, num_base_labels, space_id, lm, lmwt, wip, oov_penalty, counts, L);
  c.sp.o.timesteps = sc && nbest > 0 && opts ? opts->timesteps : nullptr;
  GramStream& gs = c.sp.s;
  gs.rows = reinterpret_cast<unsigned char*>(state); gs.row_bytes = row_bytes; gs.off_lm = SL.off_lm; gs.off_nodes = SL.off_nodes;
  gs.frames_done = frames_done;
  gs.cfg.magic = kGramStreamMagic; gs.cfg.V = V; gs.cfg.K = max_order; gs.cfg.R = sc ? num_base_labels : 0; gs.cfg.W = beam_width;
  gs.cfg.scored = sc ? 1 : 0; gs.cfg.has_lm = lm ? 1 : 0; gs.cfg.restricted = restricted ? 1 : 0; gs.cfg.max_frames = max_frames;
  hipStream_t hs = (hipStream_t)stream;
  if (const int rc = launch_cut_lists(c, q.b, workspace, cl, S, cutoff_top_n, cutoff_prob, hs)) return rc;
  const dim3 g(B), t(kBeamThreads);
  if (!sc) hipLaunchKernelGGL((gram_beam_kernel<false, false, false, true, true>), g, t, 0, hs, c);
  else if (!restricted) hipLaunchKernelGGL((gram_beam_kernel<true, false, false, true, true>), g, t, 0, hs, c);
  else hipLaunchKernelGGL((gram_beam_kernel<true, true, false, true, true>), g, t, 0, hs, c);
  E2E_HIP_CHECK(hipGetLastError(), "gram_beam_kernel (pruned stream) launch");
  return E2E_OK;
}

}  // extern "C"
