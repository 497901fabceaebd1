// ASG prefix beam search: the unpruned instances of asg_beam_kernel and their entries (e2e_asg_beam_nbest, _opt, _stream).
// The account of the search, the kernel and the host code shared with the pruned entries (asg_beam_cut.hip) are in asg_beam.h.
#include "asg_beam.h"

using namespace e2e;

extern "C" {

int e2e_asg_beam_max_width(int V) {
  if (V < 1 || V > kMaxV) return 0;
  const int w = kMaxPairs / V;
  return w < kMaxW ? w : kMaxW;
}

size_t e2e_asg_beam_workspace_bytes(int B, int T, int V, int beam_width, int with_lm) {
  (void)with_lm;                                                  // (the LM fields live in LDS: the workspace is the same)
  Layout L;
  if (B < 0 || !layout(T, V, beam_width, L)) return 0;
  return L.head + (size_t)B * L.per_utt + 256;
}

int e2e_asg_beam_nbest_opt(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV, const void* transitions,
                           const int64_t* x_len, int B, int T, int V, int num_replabels, int beam_width, int space_id,
                           const e2e_lm* lm, double lmwt, double wip, double oov_penalty,
                           int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp, double* scores,
                           int32_t* counts, void* workspace, size_t workspace_bytes, void* stream,
                           const e2e_asg_beam_opts* opts) {
  const bool restricted = opts && opts->restrict_to_lexicon != 0;
  int64_t* timesteps = opts ? opts->timesteps : nullptr;
  if (const int rc = check_beam_args(dtype, B, T, V, num_replabels, space_id, beam_width, nbest, max_out)) return rc;
  Layout L;
  if (!layout(T, V, beam_width, L)) { set_error("T=%d frames are more than the search takes", T); return E2E_ERR_UNSUPPORTED; }
  if (const int rc = check_model(lm, V, restricted)) return rc;
  if (B > 0 && (!x || !x_len || !out_len || !n_hyp || !scores || !counts || (max_out > 0 && !out))) {
    set_error("null pointer argument"); return E2E_ERR_ARG;
  }
  if (B == 0) return E2E_OK;
  if (const int rc = check_model_device(lm)) return rc;
  if (!align_workspace(workspace, workspace_bytes) || workspace_bytes < L.head + (size_t)B * L.per_utt) {
    set_error("workspace too small: %zu bytes, e2e_asg_beam_workspace_bytes() = %zu", workspace_bytes, L.head + (size_t)B * L.per_utt + 256);
    return E2E_ERR_WORKSPACE;
  }
  AsgBeamParams p;
  fill_params(p, x, dtype, sB, sT, sV, x_len, B, T, V, num_replabels, beam_width, space_id, lm, lmwt, wip, oov_penalty, nbest,
              out, max_out, out_len, n_hyp, scores, counts, timesteps, workspace, L, L.per_utt, L.off_nodes);
  auto kernel = asg_beam_kernel<false, false, false>;
  if (timesteps) kernel = restricted ? asg_beam_kernel<true, true, true> : lm ? asg_beam_kernel<true, false, true> : asg_beam_kernel<false, false, true>;
  else if (restricted) kernel = asg_beam_kernel<true, true, false>;
  else if (lm) kernel = asg_beam_kernel<true, false, false>;
  return launch(kernel, p, p, transitions, stream, "asg_beam_kernel launch");
}

int e2e_asg_beam_nbest(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV, const void* transitions,
                       const int64_t* x_len, int B, int T, int V, int num_replabels, int beam_width, int space_id,
                       const e2e_lm* lm, double lmwt, double wip, double oov_penalty,
                       int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp, double* scores,
                       int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  return e2e_asg_beam_nbest_opt(x, dtype, sB, sT, sV, transitions, x_len, B, T, V, num_replabels, beam_width, space_id, lm, lmwt,
                                wip, oov_penalty, nbest, out, max_out, out_len, n_hyp, scores, counts, workspace,
                                workspace_bytes, stream, nullptr);
}

size_t e2e_asg_beam_stream_row_bytes(int max_frames, int V, int beam_width, int with_lm) {
  StreamLayout S;
  return stream_layout(max_frames, V, beam_width, with_lm != 0, S) ? S.total : 0;
}

size_t e2e_asg_beam_stream_workspace_bytes(int B, int V, int beam_width, int with_lm) {
  (void)with_lm;
  Layout L;
  if (B < 0 || !layout(1, V, beam_width, L)) return 0;
  return L.head + (size_t)B * L.off_nodes + 256;                  // (the node pool lives in the row)
}

int e2e_asg_beam_stream(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV, const void* transitions,
                        const int64_t* chunk_len, int B, int T, int V, int num_replabels, int beam_width, int space_id,
                        const e2e_lm* lm, double lmwt, double wip, double oov_penalty,
                        void* state, size_t row_bytes, int max_frames,
                        int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp, double* scores,
                        int32_t* counts, int64_t* frames_done,
                        void* workspace, size_t workspace_bytes, void* stream, const e2e_asg_beam_opts* opts) {
  const bool restricted = opts && opts->restrict_to_lexicon != 0;
  // every argument error the host can see, before any launch
  if (const int rc = check_beam_args(dtype, B, T, V, num_replabels, space_id, beam_width, nbest, max_out, 0)) return rc;
  if (max_frames < 1 || max_frames > (1 << 22)) { set_error("max_frames=%d outside [1, %d]", max_frames, 1 << 22); return E2E_ERR_ARG; }
  StreamLayout S;
  Layout L;
  if (!stream_layout(max_frames, V, beam_width, lm != nullptr, S) || !layout(1, V, beam_width, L)) {
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
  if (!align_workspace(workspace, workspace_bytes) || workspace_bytes < L.head + (size_t)B * per_utt) {
    set_error("workspace too small: %zu bytes, e2e_asg_beam_stream_workspace_bytes() = %zu", workspace_bytes, L.head + (size_t)B * per_utt + 256);
    return E2E_ERR_WORKSPACE;
  }
  if (const int rc = check_model_device(lm)) return rc;
  AsgStreamParams sp;
  fill_params(sp.b, x, dtype, sB, sT, sV, chunk_len, B, T, V, num_replabels, beam_width, space_id, lm, lmwt, wip, oov_penalty, nbest,
              out, nbest > 0 ? max_out : 0, out_len, n_hyp, scores, counts, nbest > 0 && opts ? opts->timesteps : nullptr,
              workspace, L, per_utt, 0);
  sp.s.rows = reinterpret_cast<unsigned char*>(state); sp.s.row_bytes = row_bytes; sp.s.off_lm = S.off_lm; sp.s.off_nodes = S.off_nodes;
  sp.s.max_frames = max_frames; sp.s.frames_done = frames_done;
  auto kernel = asg_beam_kernel<false, false, false, true>;
  if (restricted) kernel = asg_beam_kernel<true, true, false, true>;
  else if (lm) kernel = asg_beam_kernel<true, false, false, true>;
  return launch(kernel, sp, sp.b, transitions, stream, "asg_beam_kernel (stream) launch");
}

}  // extern "C"
