// ASG beam search with per-frame label pruning (cutoff_top_n): e2e_asg_beam_nbest_cut and e2e_asg_beam_stream_cut.  The
// definition is in include/e2e_ctc.h beside e2e_asg_beam_nbest_opt, the account in DESIGN.md 4.10, Pruned.
//
// A call is three kernels on the caller's stream: the selection (launch_label_cut, ctc_label_cut.hip, without a blank and with
// cutoff_prob 1) writes every frame's K = min(cutoff_top_n, V) kept labels, ascending, into the head of the workspace; the
// transitions are transposed behind them; and the CUT instance of asg_beam_kernel (asg_beam.h) expands the kept labels alone.
// The nine CUT instances live in this object so that they build beside the unpruned ones; they share one parameter block
// (AsgCutParams).  A frame's pair space is W * K, which is what ctot / sval / spos are made of; the width and alphabet limits,
// the state row and its header are the unpruned search's.
#include "asg_beam.h"

namespace e2e {
namespace beamk {
// (ctc_label_cut.hip; declared in ctc_beam_common.h, which is the CTC search's device code)
int launch_label_cut(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len, int B, int T, int V,
                     int blank, int cutoff_top_n, double cutoff_prob, int* ids, int* n, hipStream_t s);
}  // namespace beamk

namespace {

int cut_k(int V, int top_n) { return top_n < V ? top_n : V; }

// the head of the workspace: ids (B,T,K) and cnt (B,T) int32, each 256-aligned; behind them the unpruned call's layout
struct CutLists { size_t off_cnt, bytes; };
CutLists cut_lists(int B, int T, int K) {
  CutLists c;
  c.off_cnt = align_up((size_t)B * T * K * 4, 256);
  c.bytes = c.off_cnt + align_up((size_t)B * T * 4, 256);
  return c;
}

// can the selection of a pruned call of these sizes run (the queries return 0 where it cannot)
bool cut_sizes_ok(int B, int T, int top_n) { return B >= 0 && T >= 1 && top_n >= 1 && (int64_t)B * T <= 0x7fffffffLL / 2; }

int check_cut_knob(int top_n) {
  if (top_n < 1) { set_error("cutoff_top_n=%d: at least 1", top_n); return E2E_ERR_ARG; }
  return E2E_OK;
}

int check_cut_workspace(void*& workspace, size_t& workspace_bytes, size_t need, const char* query) {
  if (align_workspace(workspace, workspace_bytes) && workspace_bytes >= need) return E2E_OK;
  set_error("workspace too small: %zu bytes, %s() = %zu", workspace_bytes, query, need + 256);
  return E2E_ERR_WORKSPACE;
}

// the selection into the head of the workspace, the transitions behind it, then the search
template <typename Kernel>
int launch_cut(Kernel kernel, AsgCutParams& c, const void* transitions, void* workspace, const CutLists& cl, int top_n,
               void* stream, const char* what) {
  const AsgBeamParams& p = c.sp.b;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
  int* ids = reinterpret_cast<int*>(w);
  c.ids = ids; c.K = cut_k(p.V, top_n);
  if (const int rc = beamk::launch_label_cut(p.x, p.dtype, p.sB, p.sT, p.sV, p.x_len, p.B, p.T, p.V, -1, top_n, 1.0, ids,
                                             reinterpret_cast<int*>(w + cl.off_cnt), s)) return rc;
  return launch(kernel, c, p, transitions, stream, what);
}

}  // namespace
}  // namespace e2e

using namespace e2e;

extern "C" {

size_t e2e_asg_beam_cut_workspace_bytes(int B, int T, int V, int beam_width, int with_lm, int cutoff_top_n) {
  if (cutoff_top_n < 1 || V < 1) return 0;
  if (cutoff_top_n >= V) return e2e_asg_beam_workspace_bytes(B, T, V, beam_width, with_lm);
  Layout L;
  if (!cut_sizes_ok(B, T, cutoff_top_n) || !layout(T, V, beam_width, L, cutoff_top_n)) return 0;
  return cut_lists(B, T, cutoff_top_n).bytes + L.head + (size_t)B * L.per_utt + 256;
}

size_t e2e_asg_beam_cut_stream_workspace_bytes(int B, int T, int V, int beam_width, int with_lm, int cutoff_top_n) {
  if (cutoff_top_n < 1 || V < 1 || T < 1) return 0;
  if (cutoff_top_n >= V) return e2e_asg_beam_stream_workspace_bytes(B, V, beam_width, with_lm);
  Layout L;
  if (!cut_sizes_ok(B, T, cutoff_top_n) || !layout(1, V, beam_width, L, cutoff_top_n)) return 0;
  return cut_lists(B, T, cutoff_top_n).bytes + L.head + (size_t)B * L.off_nodes + 256;     // (the node pool lives in the row)
}

int e2e_asg_beam_nbest_cut(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV, const void* transitions,
                           const int64_t* x_len, int B, int T, int V, int num_replabels, int beam_width, int space_id,
                           const e2e_lm* lm, double lmwt, double wip, double oov_penalty,
                           int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp, double* scores,
                           int32_t* counts, void* workspace, size_t workspace_bytes, void* stream,
                           const e2e_asg_beam_opts* opts, int cutoff_top_n) {
  // every argument error the host can see, before any launch
  if (const int rc = check_cut_knob(cutoff_top_n)) return rc;
  if (V >= 1 && cutoff_top_n >= V)                               // no pruning: the unpruned entry, kernel and workspace
    return e2e_asg_beam_nbest_opt(x, dtype, sB, sT, sV, transitions, x_len, B, T, V, num_replabels, beam_width, space_id, lm, lmwt,
                                  wip, oov_penalty, nbest, out, max_out, out_len, n_hyp, scores, counts, workspace,
                                  workspace_bytes, stream, opts);
  const bool restricted = opts && opts->restrict_to_lexicon != 0;
  int64_t* timesteps = opts ? opts->timesteps : nullptr;
  if (const int rc = check_beam_args(dtype, B, T, V, num_replabels, space_id, beam_width, nbest, max_out)) return rc;
  const int K = cut_k(V, cutoff_top_n);
  Layout L;
  if (!cut_sizes_ok(B, T, cutoff_top_n) || !layout(T, V, beam_width, L, K)) {
    set_error("T=%d frames are more than the search takes", T); return E2E_ERR_UNSUPPORTED;
  }
  if (const int rc = check_model(lm, V, restricted)) return rc;
  if (B > 0 && (!x || !x_len || !out_len || !n_hyp || !scores || !counts || (max_out > 0 && !out))) {
    set_error("null pointer argument"); return E2E_ERR_ARG;
  }
  if (B == 0) return E2E_OK;
  if (const int rc = check_model_device(lm)) return rc;
  const CutLists cl = cut_lists(B, T, K);
  if (const int rc = check_cut_workspace(workspace, workspace_bytes, cl.bytes + L.head + (size_t)B * L.per_utt,
                                         "e2e_asg_beam_cut_workspace_bytes")) return rc;
  AsgCutParams c;
  memset(&c, 0, sizeof(c));
  fill_params(c.sp.b, x, dtype, sB, sT, sV, x_len, B, T, V, num_replabels, beam_width, space_id, lm, lmwt, wip, oov_penalty, nbest,
              out, max_out, out_len, n_hyp, scores, counts, timesteps, reinterpret_cast<unsigned char*>(workspace) + cl.bytes, L,
              L.per_utt, L.off_nodes);
  auto kernel = asg_beam_kernel<false, false, false, false, true>;
  if (timesteps) kernel = restricted ? asg_beam_kernel<true, true, true, false, true>
                          : lm ? asg_beam_kernel<true, false, true, false, true> : asg_beam_kernel<false, false, true, false, true>;
  else if (restricted) kernel = asg_beam_kernel<true, true, false, false, true>;
  else if (lm) kernel = asg_beam_kernel<true, false, false, false, true>;
  return launch_cut(kernel, c, transitions, workspace, cl, cutoff_top_n, stream, "asg_beam_kernel (pruned) launch");
}

int e2e_asg_beam_stream_cut(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV, const void* transitions,
                            const int64_t* chunk_len, int B, int T, int V, int num_replabels, int beam_width, int space_id,
                            const e2e_lm* lm, double lmwt, double wip, double oov_penalty,
                            void* state, size_t row_bytes, int max_frames,
                            int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp, double* scores,
                            int32_t* counts, int64_t* frames_done,
                            void* workspace, size_t workspace_bytes, void* stream, const e2e_asg_beam_opts* opts,
                            int cutoff_top_n) {
  if (const int rc = check_cut_knob(cutoff_top_n)) return rc;
  if (V >= 1 && cutoff_top_n >= V)
    return e2e_asg_beam_stream(x, dtype, sB, sT, sV, transitions, chunk_len, B, T, V, num_replabels, beam_width, space_id, lm, lmwt,
                               wip, oov_penalty, state, row_bytes, max_frames, nbest, out, max_out, out_len, n_hyp, scores, counts,
                               frames_done, workspace, workspace_bytes, stream, opts);
  const bool restricted = opts && opts->restrict_to_lexicon != 0;
  if (const int rc = check_beam_args(dtype, B, T, V, num_replabels, space_id, beam_width, nbest, max_out, 0)) return rc;
  if (max_frames < 1 || max_frames > (1 << 22)) { set_error("max_frames=%d outside [1, %d]", max_frames, 1 << 22); return E2E_ERR_ARG; }
  const int K = cut_k(V, cutoff_top_n);
  StreamLayout S;
  Layout L;
  if (!cut_sizes_ok(B, T, cutoff_top_n) || !stream_layout(max_frames, V, beam_width, lm != nullptr, S) || !layout(1, V, beam_width, L, K)) {
    set_error("max_frames=%d frames are more than the search takes", max_frames); return E2E_ERR_UNSUPPORTED;
  }
  if (const int rc = check_row_bytes(row_bytes, S.total, "e2e_asg_beam_stream_row_bytes")) return rc;
  if (const int rc = check_model(lm, V, restricted)) return rc;
  if (B > 0 && (!x || !chunk_len || !state || !frames_done)) { set_error("null pointer argument"); return E2E_ERR_ARG; }
  if (B > 0 && nbest > 0 && (!out_len || !n_hyp || !scores || !counts || (max_out > 0 && !out))) {
    set_error("null pointer argument"); return E2E_ERR_ARG;
  }
  if (const int rc = check_state_aligned(B, state)) return rc;
  if (B == 0) return E2E_OK;
  const size_t per_utt = L.off_nodes;                             // (the node pool lives in the row)
  const CutLists cl = cut_lists(B, T, K);
  if (const int rc = check_cut_workspace(workspace, workspace_bytes, cl.bytes + L.head + (size_t)B * per_utt,
                                         "e2e_asg_beam_cut_stream_workspace_bytes")) return rc;
  if (const int rc = check_model_device(lm)) return rc;
  AsgCutParams c;
  memset(&c, 0, sizeof(c));
  fill_params(c.sp.b, x, dtype, sB, sT, sV, chunk_len, B, T, V, num_replabels, beam_width, space_id, lm, lmwt, wip, oov_penalty,
              nbest, out, nbest > 0 ? max_out : 0, out_len, n_hyp, scores, counts, nbest > 0 && opts ? opts->timesteps : nullptr,
              reinterpret_cast<unsigned char*>(workspace) + cl.bytes, L, per_utt, 0);
  AsgStream& as = c.sp.s;
  as.rows = reinterpret_cast<unsigned char*>(state); as.row_bytes = row_bytes; as.off_lm = S.off_lm; as.off_nodes = S.off_nodes;
  as.max_frames = max_frames; as.frames_done = frames_done;
  auto kernel = asg_beam_kernel<false, false, false, true, true>;
  if (restricted) kernel = asg_beam_kernel<true, true, false, true, true>;
  else if (lm) kernel = asg_beam_kernel<true, false, false, true, true>;
  return launch_cut(kernel, c, transitions, workspace, cl, cutoff_top_n, stream, "asg_beam_kernel (pruned stream) launch");
}

}  // extern "C"
