// end2end_amd._C -- the thin pybind11 layer between the Python host code and the C ABI of libe2e_ctc.so
// (include/e2e_ctc.h).  It stands where the reference's pybind modules stand (src/losses/ctc_loss_py.cpp:5-17,
// src/decoders/ctc_decoder_py.cpp:5-39) but carries no tensor types: the Python side hands device addresses
// (tensor.data_ptr()), strides and sizes; every function forwards to exactly one extern "C" entry point and turns a
// negative return code into the Python exception E2EError carrying e2e_last_error().
//
// Compiled with plain g++ against the pybind11 headers (no torch headers, no HIP headers): end2end_amd/csrc/Makefile.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/e2e_ctc.h"

namespace py = pybind11;

namespace {

struct E2EError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

inline void check(int rc) {
  if (rc != E2E_OK) throw E2EError(std::string("libe2e_ctc: ") + e2e_last_error() + " (code " + std::to_string(rc) + ")");
}

template <typename T>
inline T* ptr(uintptr_t a) { return reinterpret_cast<T*>(a); }

// Owner of an e2e_lm handle (the decoder owns its KenLM model through a unique_ptr upstream, ctc_decoder.h:51).
class LanguageModel {
 public:
  LanguageModel(const std::string& path, const std::vector<std::string>& labels, bool case_sensitive) {
    std::vector<const char*> c;
    c.reserve(labels.size());
    for (const auto& s : labels) c.push_back(s.c_str());
    check(e2e_lm_load_arpa(path.c_str(), c.data(), (int)c.size(), case_sensitive ? 1 : 0, &lm_));
  }
  // the model that scores nothing, from a word list (e2e_lm_load_words)
  struct FromWords {};
  LanguageModel(FromWords, const std::vector<std::string>& words, const std::vector<std::string>& labels, bool case_sensitive) {
    std::vector<const char*> w, c;
    for (const auto& s : words) w.push_back(s.c_str());
    for (const auto& s : labels) c.push_back(s.c_str());
    check(e2e_lm_load_words(w.data(), (int)w.size(), c.data(), (int)c.size(), case_sensitive ? 1 : 0, &lm_));
  }
  // a model keyed by custom transcriptions (e2e_lm_load_transcriptions); path "": the model that scores nothing
  struct FromTranscriptions {};
  LanguageModel(FromTranscriptions, const std::string& path, const std::vector<std::string>& words,
                const std::vector<int32_t>& label_ids, const std::vector<int32_t>& offsets,
                const std::vector<std::string>& labels, bool case_sensitive) {
    if (offsets.size() != words.size() + 1 || (int64_t)label_ids.size() != (offsets.empty() ? 0 : offsets.back()))
      throw E2EError("libe2e_ctc: transcriptions: offsets must have one entry per word and one more, the last the number of label ids");
    std::vector<const char*> w, c;
    for (const auto& s : words) w.push_back(s.c_str());
    for (const auto& s : labels) c.push_back(s.c_str());
    check(e2e_lm_load_transcriptions(path.empty() ? nullptr : path.c_str(), w.data(), label_ids.data(), offsets.data(),
                                     (int)w.size(), c.data(), (int)c.size(), case_sensitive ? 1 : 0, &lm_));
  }
  ~LanguageModel() { e2e_lm_free(lm_); }
  LanguageModel(const LanguageModel&) = delete;
  LanguageModel& operator=(const LanguageModel&) = delete;

  uintptr_t handle() const { return reinterpret_cast<uintptr_t>(lm_); }
  int order() const { return e2e_lm_order(lm_); }
  int device() const { return e2e_lm_device(lm_); }
  uint32_t word_index(const std::string& w) const { return e2e_lm_word_index(lm_, w.c_str()); }
  void enable_lexicon() { check(e2e_lm_enable_lexicon(lm_)); }
  bool has_lexicon() const { return e2e_lm_has_lexicon(lm_) != 0; }
  int spelling_class(const std::string& s) const { return e2e_lm_spelling_class(lm_, s.c_str()); }
  double score(const std::vector<uint32_t>& ctx, uint32_t word) const {
    return e2e_lm_score(lm_, ctx.data(), (int)ctx.size(), word);
  }
  bool is_transcribed() const { return e2e_lm_is_transcribed(lm_) != 0; }
  int transcriptions_dropped() const { return e2e_lm_transcriptions_dropped(lm_); }
  std::vector<uint32_t> transcribe(const std::vector<int64_t>& ids, int space_id) const {
    std::vector<uint32_t> out(ids.size() + 1);
    int n = 0;
    check(e2e_lm_transcribe(lm_, ids.data(), (int64_t)ids.size(), space_id, out.data(), (int)out.size(), &n));
    out.resize((size_t)n);
    return out;
  }
  py::object word_string(uint32_t id) const {
    const char* s = e2e_lm_word_string(lm_, id);
    return s ? py::object(py::str(s)) : py::object(py::none());
  }

 private:
  e2e_lm* lm_ = nullptr;
};

}  // namespace

PYBIND11_MODULE(_C, m) {
  m.doc() = "pybind11 layer over the C ABI of libe2e_ctc.so (include/e2e_ctc.h): addresses and sizes in, exceptions out";
  py::register_exception<E2EError>(m, "E2EError", PyExc_RuntimeError);

  m.attr("ABI_VERSION") = E2E_CTC_ABI_VERSION;
  m.attr("F32") = E2E_F32;
  m.attr("F64") = E2E_F64;
  m.attr("F16") = E2E_F16;
  m.attr("BF16") = E2E_BF16;
  m.attr("ERR_UNSUPPORTED") = E2E_ERR_UNSUPPORTED;
  m.attr("ALGO_AUTO") = E2E_ALGO_AUTO;
  m.attr("ALGO_EXACT") = E2E_ALGO_EXACT;
  m.attr("ALGO_FAST") = E2E_ALGO_FAST;
  m.attr("REDUCE_NONE") = E2E_REDUCE_NONE;
  m.attr("REDUCE_SUM") = E2E_REDUCE_SUM;
  m.attr("REDUCE_MEAN") = E2E_REDUCE_MEAN;
  m.attr("CHAINS_F64") = E2E_CHAINS_F64;
  m.attr("CHAINS_F32") = E2E_CHAINS_F32;

  m.def("abi_version", [] { return e2e_ctc_abi_version(); });
  m.def("last_error", [] { return std::string(e2e_last_error()); });

  m.def("ctc_loss_workspace_bytes", [](int B, int T, int V, int Smax, int dtype, int algo) {
    return e2e_ctc_loss_workspace_bytes(B, T, V, Smax, dtype, algo);
  });

  m.def("ctc_loss_takes_dtype", [](int dtype, int algo, int T, int V, int Smax, int64_t sB, int64_t sT, int64_t sV, uintptr_t x, uintptr_t grads) {
    return e2e_ctc_loss_takes_dtype(dtype, algo, T, V, Smax, sB, sT, sV, reinterpret_cast<const void*>(x), reinterpret_cast<const void*>(grads)) != 0;
  });

  // (grad_scale / reduced / reduction / chains: e2e_ctc_loss_opts; the defaults are the plain call)
  m.def("ctc_loss_fwd_bwd",
        [](uintptr_t x, int dtype, bool input_is_logprobs, int64_t sB, int64_t sT, int64_t sV, uintptr_t targets,
           int64_t tgt_stride, uintptr_t x_len, uintptr_t t_len, int B, int T, int V, int Smax, int blank,
           uintptr_t losses, uintptr_t grads, uintptr_t workspace, size_t workspace_bytes, int algo, uintptr_t stream,
           double grad_scale, uintptr_t reduced, int reduction, int chains) {
          e2e_ctc_loss_opts o{grad_scale, ptr<void>(reduced), reduction, chains};
          check(e2e_ctc_loss_fwd_bwd_opt(ptr<const void>(x), dtype, input_is_logprobs ? 1 : 0, sB, sT, sV,
                                         ptr<const int64_t>(targets), tgt_stride, ptr<const int64_t>(x_len),
                                         ptr<const int64_t>(t_len), B, T, V, Smax, blank, ptr<void>(losses),
                                         ptr<void>(grads), ptr<void>(workspace), workspace_bytes, algo,
                                         ptr<void>(stream), &o));
        },
        py::arg("x"), py::arg("dtype"), py::arg("input_is_logprobs"), py::arg("sB"), py::arg("sT"), py::arg("sV"),
        py::arg("targets"), py::arg("tgt_stride"), py::arg("x_len"), py::arg("t_len"), py::arg("B"), py::arg("T"),
        py::arg("V"), py::arg("Smax"), py::arg("blank"), py::arg("losses"), py::arg("grads"), py::arg("workspace"),
        py::arg("workspace_bytes"), py::arg("algo"), py::arg("stream"), py::arg("grad_scale") = 1.0,
        py::arg("reduced") = 0, py::arg("reduction") = E2E_REDUCE_NONE, py::arg("chains") = E2E_CHAINS_F64);

  m.def("ctc_noblank_workspace_bytes", [](int B, int T, int V, int Smax, int dtype) {
    return e2e_ctc_noblank_workspace_bytes(B, T, V, Smax, dtype);
  });

  // (arguments the library would refuse are refused here too, before anything reaches the GPU)
  m.def("ctc_noblank_fwd_bwd",
        [](uintptr_t x, int dtype, bool input_is_logprobs, int64_t sB, int64_t sT, int64_t sV, uintptr_t targets,
           int64_t tgt_stride, uintptr_t x_len, uintptr_t t_len, int B, int T, int V, int Smax, int space_idx,
           uintptr_t losses, uintptr_t grads, uintptr_t workspace, size_t workspace_bytes, uintptr_t stream,
           double grad_scale, uintptr_t reduced, int reduction) {
          if (dtype != E2E_F32 && dtype != E2E_F64) throw py::value_error("ctc_noblank_fwd_bwd: dtype must be F32 or F64");
          if (V < 1 || (space_idx != -1 && (space_idx < 0 || space_idx >= V)))
            throw py::value_error("ctc_noblank_fwd_bwd: space_idx " + std::to_string(space_idx) + " is neither -1 nor in [0, " +
                                  std::to_string(V) + ")");
          if (reduction < E2E_REDUCE_NONE || reduction > E2E_REDUCE_MEAN || (reduction != E2E_REDUCE_NONE && !reduced))
            throw py::value_error("ctc_noblank_fwd_bwd: bad reduction");
          e2e_ctc_loss_opts o{grad_scale, ptr<void>(reduced), reduction, E2E_CHAINS_F64};
          check(e2e_ctc_noblank_fwd_bwd(ptr<const void>(x), dtype, input_is_logprobs ? 1 : 0, sB, sT, sV,
                                        ptr<const int64_t>(targets), tgt_stride, ptr<const int64_t>(x_len),
                                        ptr<const int64_t>(t_len), B, T, V, Smax, space_idx, ptr<void>(losses),
                                        ptr<void>(grads), ptr<void>(workspace), workspace_bytes, ptr<void>(stream), &o));
        },
        py::arg("x"), py::arg("dtype"), py::arg("input_is_logprobs"), py::arg("sB"), py::arg("sT"), py::arg("sV"),
        py::arg("targets"), py::arg("tgt_stride"), py::arg("x_len"), py::arg("t_len"), py::arg("B"), py::arg("T"),
        py::arg("V"), py::arg("Smax"), py::arg("space_idx"), py::arg("losses"), py::arg("grads"), py::arg("workspace"),
        py::arg("workspace_bytes"), py::arg("stream"), py::arg("grad_scale") = 1.0, py::arg("reduced") = 0,
        py::arg("reduction") = E2E_REDUCE_NONE);

  m.def("gram_ctc_workspace_bytes", [](int B, int T, int V, int Smax, int max_order, int dtype) {
    return e2e_gram_ctc_workspace_bytes(B, T, V, Smax, max_order, dtype);
  });

  m.def("gram_ctc_fwd_bwd",
        [](uintptr_t x, int dtype, bool input_is_logprobs, int64_t sB, int64_t sT, int64_t sV, uintptr_t targets,
           int64_t tgt_stride, uintptr_t x_len, uintptr_t t_len, int B, int T, int V, int Smax, uintptr_t keys,
           uintptr_t cols, int n_grams, int radix, int max_order, uintptr_t losses, uintptr_t grads, uintptr_t workspace,
           size_t workspace_bytes, uintptr_t stream, double grad_scale, uintptr_t reduced, int reduction) {
          if (dtype != E2E_F32 && dtype != E2E_F64) throw py::value_error("gram_ctc_fwd_bwd: dtype must be F32 or F64");
          if (radix < 1 || radix > V)
            throw py::value_error("gram_ctc_fwd_bwd: radix " + std::to_string(radix) + " is not in [1, " + std::to_string(V) + "]");
          if (max_order < 1 || max_order > 8)
            throw py::value_error("gram_ctc_fwd_bwd: max_order " + std::to_string(max_order) + " is not in [1, 8]");
          if (n_grams < 0 || (n_grams > 0 && (!keys || !cols))) throw py::value_error("gram_ctc_fwd_bwd: bad gram table");
          if (reduction < E2E_REDUCE_NONE || reduction > E2E_REDUCE_MEAN || (reduction != E2E_REDUCE_NONE && !reduced))
            throw py::value_error("gram_ctc_fwd_bwd: bad reduction");
          e2e_ctc_loss_opts o{grad_scale, ptr<void>(reduced), reduction, E2E_CHAINS_F64};
          check(e2e_gram_ctc_fwd_bwd(ptr<const void>(x), dtype, input_is_logprobs ? 1 : 0, sB, sT, sV,
                                     ptr<const int64_t>(targets), tgt_stride, ptr<const int64_t>(x_len),
                                     ptr<const int64_t>(t_len), B, T, V, Smax, ptr<const int64_t>(keys),
                                     ptr<const int32_t>(cols), n_grams, radix, max_order, ptr<void>(losses),
                                     ptr<void>(grads), ptr<void>(workspace), workspace_bytes, ptr<void>(stream), &o));
        },
        py::arg("x"), py::arg("dtype"), py::arg("input_is_logprobs"), py::arg("sB"), py::arg("sT"), py::arg("sV"),
        py::arg("targets"), py::arg("tgt_stride"), py::arg("x_len"), py::arg("t_len"), py::arg("B"), py::arg("T"),
        py::arg("V"), py::arg("Smax"), py::arg("keys"), py::arg("cols"), py::arg("n_grams"), py::arg("radix"),
        py::arg("max_order"), py::arg("losses"), py::arg("grads"), py::arg("workspace"), py::arg("workspace_bytes"),
        py::arg("stream"), py::arg("grad_scale") = 1.0, py::arg("reduced") = 0, py::arg("reduction") = E2E_REDUCE_NONE);

  m.def("asg_max_labels", [] { return e2e_asg_max_labels(); });
  m.def("asg_max_target_length", [] { return e2e_asg_max_target_length(); });
  m.def("asg_workspace_bytes", [](int B, int T, int V, int Smax, int dtype) {
    return e2e_asg_workspace_bytes(B, T, V, Smax, dtype);
  });

  m.def("asg_fwd_bwd",
        [](uintptr_t x, int dtype, int64_t sB, int64_t sT, int64_t sV, uintptr_t transitions, uintptr_t targets,
           int64_t tgt_stride, uintptr_t x_len, uintptr_t t_len, int B, int T, int V, int Smax, uintptr_t losses,
           uintptr_t grads, uintptr_t tgrads, uintptr_t workspace, size_t workspace_bytes, uintptr_t stream,
           double grad_scale) {
          if (dtype != E2E_F32 && dtype != E2E_F64) throw py::value_error("asg_fwd_bwd: dtype must be F32 or F64");
          e2e_ctc_loss_opts o{grad_scale, nullptr, E2E_REDUCE_NONE, E2E_CHAINS_F64};
          check(e2e_asg_fwd_bwd(ptr<const void>(x), dtype, sB, sT, sV, ptr<const void>(transitions),
                                ptr<const int64_t>(targets), tgt_stride, ptr<const int64_t>(x_len),
                                ptr<const int64_t>(t_len), B, T, V, Smax, ptr<void>(losses), ptr<void>(grads),
                                ptr<void>(tgrads), ptr<void>(workspace), workspace_bytes, ptr<void>(stream), &o));
        },
        py::arg("x"), py::arg("dtype"), py::arg("sB"), py::arg("sT"), py::arg("sV"), py::arg("transitions"),
        py::arg("targets"), py::arg("tgt_stride"), py::arg("x_len"), py::arg("t_len"), py::arg("B"), py::arg("T"),
        py::arg("V"), py::arg("Smax"), py::arg("losses"), py::arg("grads"), py::arg("tgrads"), py::arg("workspace"),
        py::arg("workspace_bytes"), py::arg("stream"), py::arg("grad_scale") = 1.0);

  m.def("asg_viterbi_workspace_bytes", [](int B, int T, int V) { return e2e_asg_viterbi_workspace_bytes(B, T, V); });

  m.def("asg_viterbi",
        [](uintptr_t x, int dtype, int64_t sB, int64_t sT, int64_t sV, uintptr_t transitions, uintptr_t x_len, int B,
           int T, int V, uintptr_t path, int64_t pad_value, uintptr_t scores, uintptr_t collapsed, uintptr_t lengths,
           uintptr_t workspace, size_t workspace_bytes, uintptr_t stream) {
          check(e2e_asg_viterbi(ptr<const void>(x), dtype, sB, sT, sV, ptr<const void>(transitions),
                                ptr<const int64_t>(x_len), B, T, V, ptr<int64_t>(path), pad_value, ptr<double>(scores),
                                ptr<int64_t>(collapsed), ptr<int64_t>(lengths), ptr<void>(workspace), workspace_bytes,
                                ptr<void>(stream)));
        },
        py::arg("x"), py::arg("dtype"), py::arg("sB"), py::arg("sT"), py::arg("sV"), py::arg("transitions"),
        py::arg("x_len"), py::arg("B"), py::arg("T"), py::arg("V"), py::arg("path"), py::arg("pad_value"),
        py::arg("scores"), py::arg("collapsed"), py::arg("lengths"), py::arg("workspace"), py::arg("workspace_bytes"),
        py::arg("stream"));

  m.def("gram_ctc_greedy",
        [](uintptr_t x, int dtype, int64_t sB, int64_t sT, int64_t sV, uintptr_t x_len, int B, int T, int V,
           uintptr_t gram_ids, uintptr_t gram_len, int max_order, uintptr_t out, uintptr_t out_len, uintptr_t cols,
           uintptr_t cols_len, uintptr_t stream) {
          check(e2e_gram_ctc_greedy(ptr<const void>(x), dtype, sB, sT, sV, ptr<const int64_t>(x_len), B, T, V,
                                    ptr<const int32_t>(gram_ids), ptr<const int32_t>(gram_len), max_order,
                                    ptr<int64_t>(out), ptr<int64_t>(out_len), ptr<int64_t>(cols), ptr<int64_t>(cols_len),
                                    ptr<void>(stream)));
        },
        py::arg("x"), py::arg("dtype"), py::arg("sB"), py::arg("sT"), py::arg("sV"), py::arg("x_len"), py::arg("B"),
        py::arg("T"), py::arg("V"), py::arg("gram_ids"), py::arg("gram_len"), py::arg("max_order"), py::arg("out"),
        py::arg("out_len"), py::arg("cols"), py::arg("cols_len"), py::arg("stream"));

  m.def("gram_beam_max_width", [](int V, int max_order) { return e2e_gram_beam_max_width(V, max_order); });
  m.def("gram_beam_workspace_bytes", [](int B, int T, int V, int max_order, int beam_width) {
    return e2e_gram_beam_workspace_bytes(B, T, V, max_order, beam_width);
  });

  m.def("gram_ctc_beam_nbest",
        [](uintptr_t lp, int dtype, int64_t sB, int64_t sT, int64_t sV, uintptr_t x_len, int B, int T, int V,
           uintptr_t gram_ids, uintptr_t gram_len, int max_order, int beam_width, int nbest, uintptr_t out,
           int64_t max_out, uintptr_t out_len, uintptr_t n_hyp, uintptr_t scores, uintptr_t workspace,
           size_t workspace_bytes, uintptr_t stream) {
          check(e2e_gram_ctc_beam_nbest(ptr<const void>(lp), dtype, sB, sT, sV, ptr<const int64_t>(x_len), B, T, V,
                                        ptr<const int32_t>(gram_ids), ptr<const int32_t>(gram_len), max_order,
                                        beam_width, nbest, ptr<int64_t>(out), max_out, ptr<int64_t>(out_len),
                                        ptr<int64_t>(n_hyp), ptr<double>(scores), ptr<void>(workspace), workspace_bytes,
                                        ptr<void>(stream)));
        },
        py::arg("lp"), py::arg("dtype"), py::arg("sB"), py::arg("sT"), py::arg("sV"), py::arg("x_len"), py::arg("B"),
        py::arg("T"), py::arg("V"), py::arg("gram_ids"), py::arg("gram_len"), py::arg("max_order"),
        py::arg("beam_width"), py::arg("nbest"), py::arg("out"), py::arg("max_out"), py::arg("out_len"),
        py::arg("n_hyp"), py::arg("scores"), py::arg("workspace"), py::arg("workspace_bytes"), py::arg("stream"));

  m.def("gram_beam_workspace_bytes_lm", [](int B, int T, int V, int max_order, int beam_width, bool with_lm) {
    return e2e_gram_beam_workspace_bytes_lm(B, T, V, max_order, beam_width, with_lm ? 1 : 0);
  });

  m.def("gram_ctc_beam_nbest_lm",
        [](uintptr_t lp, int dtype, int64_t sB, int64_t sT, int64_t sV, uintptr_t x_len, int B, int T, int V,
           uintptr_t gram_ids, uintptr_t gram_len, int max_order, int num_base_labels, int beam_width, int space_id,
           uintptr_t lm, double lmwt, double wip, double oov_penalty, int nbest, uintptr_t out, int64_t max_out,
           uintptr_t out_len, uintptr_t n_hyp, uintptr_t scores, uintptr_t counts, uintptr_t workspace,
           size_t workspace_bytes, uintptr_t stream) {
          check(e2e_gram_ctc_beam_nbest_lm(ptr<const void>(lp), dtype, sB, sT, sV, ptr<const int64_t>(x_len), B, T, V,
                                           ptr<const int32_t>(gram_ids), ptr<const int32_t>(gram_len), max_order,
                                           num_base_labels, beam_width, space_id, ptr<const e2e_lm>(lm), lmwt, wip,
                                           oov_penalty, nbest, ptr<int64_t>(out), max_out, ptr<int64_t>(out_len),
                                           ptr<int64_t>(n_hyp), ptr<double>(scores), ptr<int32_t>(counts),
                                           ptr<void>(workspace), workspace_bytes, ptr<void>(stream)));
        },
        py::arg("lp"), py::arg("dtype"), py::arg("sB"), py::arg("sT"), py::arg("sV"), py::arg("x_len"), py::arg("B"),
        py::arg("T"), py::arg("V"), py::arg("gram_ids"), py::arg("gram_len"), py::arg("max_order"),
        py::arg("num_base_labels"), py::arg("beam_width"), py::arg("space_id"), py::arg("lm"), py::arg("lmwt"),
        py::arg("wip"), py::arg("oov_penalty"), py::arg("nbest"), py::arg("out"), py::arg("max_out"), py::arg("out_len"),
        py::arg("n_hyp"), py::arg("scores"), py::arg("counts"), py::arg("workspace"), py::arg("workspace_bytes"),
        py::arg("stream"));

  // opts: None passes NULL; else (restrict_to_lexicon, timesteps) -- zeros included, to tell the two apart
  m.def("gram_ctc_beam_nbest_opt",
        [](uintptr_t lp, int dtype, int64_t sB, int64_t sT, int64_t sV, uintptr_t x_len, int B, int T, int V,
           uintptr_t gram_ids, uintptr_t gram_len, int max_order, int num_base_labels, int beam_width, int space_id,
           uintptr_t lm, double lmwt, double wip, double oov_penalty, int nbest, uintptr_t out, int64_t max_out,
           uintptr_t out_len, uintptr_t n_hyp, uintptr_t scores, uintptr_t counts, uintptr_t workspace,
           size_t workspace_bytes, uintptr_t stream, py::object opts) {
          e2e_gram_beam_opts o{0, nullptr};
          if (!opts.is_none()) {
            auto t = opts.cast<std::pair<bool, uintptr_t>>();
            o.restrict_to_lexicon = t.first ? 1 : 0;
            o.timesteps = ptr<int64_t>(t.second);
          }
          check(e2e_gram_ctc_beam_nbest_opt(ptr<const void>(lp), dtype, sB, sT, sV, ptr<const int64_t>(x_len), B, T, V,
                                            ptr<const int32_t>(gram_ids), ptr<const int32_t>(gram_len), max_order,
                                            num_base_labels, beam_width, space_id, ptr<const e2e_lm>(lm), lmwt, wip,
                                            oov_penalty, nbest, ptr<int64_t>(out), max_out, ptr<int64_t>(out_len),
                                            ptr<int64_t>(n_hyp), ptr<double>(scores), ptr<int32_t>(counts),
                                            ptr<void>(workspace), workspace_bytes, ptr<void>(stream),
                                            opts.is_none() ? nullptr : &o));
        },
        py::arg("lp"), py::arg("dtype"), py::arg("sB"), py::arg("sT"), py::arg("sV"), py::arg("x_len"), py::arg("B"),
        py::arg("T"), py::arg("V"), py::arg("gram_ids"), py::arg("gram_len"), py::arg("max_order"),
        py::arg("num_base_labels"), py::arg("beam_width"), py::arg("space_id"), py::arg("lm"), py::arg("lmwt"),
        py::arg("wip"), py::arg("oov_penalty"), py::arg("nbest"), py::arg("out"), py::arg("max_out"), py::arg("out_len"),
        py::arg("n_hyp"), py::arg("scores"), py::arg("counts"), py::arg("workspace"), py::arg("workspace_bytes"),
        py::arg("stream"), py::arg("opts") = py::none());

  m.def("gram_beam_stream_row_bytes", [](int max_frames, int V, int max_order, int beam_width, bool scored, bool with_lm) {
    return e2e_gram_beam_stream_row_bytes(max_frames, V, max_order, beam_width, scored ? 1 : 0, with_lm ? 1 : 0);
  });
  m.def("gram_beam_stream_workspace_bytes", [](int B, int V, int max_order, int beam_width, bool scored, bool with_lm) {
    return e2e_gram_beam_stream_workspace_bytes(B, V, max_order, beam_width, scored ? 1 : 0, with_lm ? 1 : 0);
  });

  // opts: None passes NULL; else (restrict_to_lexicon, timesteps), as gram_ctc_beam_nbest_opt takes them
  m.def("gram_ctc_beam_stream",
        [](uintptr_t lp, int dtype, int64_t sB, int64_t sT, int64_t sV, uintptr_t chunk_len, int B, int T, int V,
           uintptr_t gram_ids, uintptr_t gram_len, int max_order, int num_base_labels, int beam_width, bool scored,
           int space_id, uintptr_t lm, double lmwt, double wip, double oov_penalty, uintptr_t state, size_t row_bytes,
           int max_frames, int nbest, uintptr_t out, int64_t max_out, uintptr_t out_len, uintptr_t n_hyp, uintptr_t scores,
           uintptr_t counts, uintptr_t frames_done, uintptr_t workspace, size_t workspace_bytes, uintptr_t stream,
           py::object opts) {
          e2e_gram_beam_opts o{0, nullptr};
          if (!opts.is_none()) {
            auto t = opts.cast<std::pair<bool, uintptr_t>>();
            o.restrict_to_lexicon = t.first ? 1 : 0;
            o.timesteps = ptr<int64_t>(t.second);
          }
          check(e2e_gram_ctc_beam_stream(ptr<const void>(lp), dtype, sB, sT, sV, ptr<const int64_t>(chunk_len), B, T, V,
                                         ptr<const int32_t>(gram_ids), ptr<const int32_t>(gram_len), max_order,
                                         num_base_labels, beam_width, scored ? 1 : 0, space_id, ptr<const e2e_lm>(lm), lmwt,
                                         wip, oov_penalty, ptr<void>(state), row_bytes, max_frames, nbest,
                                         ptr<int64_t>(out), max_out, ptr<int64_t>(out_len), ptr<int64_t>(n_hyp),
                                         ptr<double>(scores), ptr<int32_t>(counts), ptr<int64_t>(frames_done),
                                         ptr<void>(workspace), workspace_bytes, ptr<void>(stream),
                                         opts.is_none() ? nullptr : &o));
        },
        py::arg("lp"), py::arg("dtype"), py::arg("sB"), py::arg("sT"), py::arg("sV"), py::arg("chunk_len"), py::arg("B"),
        py::arg("T"), py::arg("V"), py::arg("gram_ids"), py::arg("gram_len"), py::arg("max_order"),
        py::arg("num_base_labels"), py::arg("beam_width"), py::arg("scored"), py::arg("space_id"), py::arg("lm"),
        py::arg("lmwt"), py::arg("wip"), py::arg("oov_penalty"), py::arg("state"), py::arg("row_bytes"),
        py::arg("max_frames"), py::arg("nbest"), py::arg("out"), py::arg("max_out"), py::arg("out_len"), py::arg("n_hyp"),
        py::arg("scores"), py::arg("counts"), py::arg("frames_done"), py::arg("workspace"), py::arg("workspace_bytes"),
        py::arg("stream"), py::arg("opts") = py::none());

  m.def("asg_beam_max_width", [](int V) { return e2e_asg_beam_max_width(V); });
  m.def("asg_beam_workspace_bytes", [](int B, int T, int V, int beam_width, bool with_lm) {
    return e2e_asg_beam_workspace_bytes(B, T, V, beam_width, with_lm ? 1 : 0);
  });

  m.def("asg_beam_nbest",
        [](uintptr_t x, int dtype, int64_t sB, int64_t sT, int64_t sV, uintptr_t transitions, uintptr_t x_len, int B,
           int T, int V, int num_replabels, int beam_width, int space_id, uintptr_t lm, double lmwt, double wip,
           double oov_penalty, int nbest, uintptr_t out, int64_t max_out, uintptr_t out_len, uintptr_t n_hyp,
           uintptr_t scores, uintptr_t counts, uintptr_t workspace, size_t workspace_bytes, uintptr_t stream,
           bool restrict_to_lexicon, uintptr_t timesteps) {
          e2e_asg_beam_opts o{restrict_to_lexicon ? 1 : 0, ptr<int64_t>(timesteps)};
          check(e2e_asg_beam_nbest_opt(ptr<const void>(x), dtype, sB, sT, sV, ptr<const void>(transitions),
                                       ptr<const int64_t>(x_len), B, T, V, num_replabels, beam_width, space_id,
                                       ptr<const e2e_lm>(lm), lmwt, wip, oov_penalty, nbest, ptr<int64_t>(out), max_out,
                                       ptr<int64_t>(out_len), ptr<int64_t>(n_hyp), ptr<double>(scores),
                                       ptr<int32_t>(counts), ptr<void>(workspace), workspace_bytes, ptr<void>(stream), &o));
        },
        py::arg("x"), py::arg("dtype"), py::arg("sB"), py::arg("sT"), py::arg("sV"), py::arg("transitions"),
        py::arg("x_len"), py::arg("B"), py::arg("T"), py::arg("V"), py::arg("num_replabels"), py::arg("beam_width"),
        py::arg("space_id"), py::arg("lm"), py::arg("lmwt"), py::arg("wip"), py::arg("oov_penalty"), py::arg("nbest"),
        py::arg("out"), py::arg("max_out"), py::arg("out_len"), py::arg("n_hyp"), py::arg("scores"), py::arg("counts"),
        py::arg("workspace"), py::arg("workspace_bytes"), py::arg("stream"), py::arg("restrict_to_lexicon") = false,
        py::arg("timesteps") = (uintptr_t)0);

  m.def("asg_beam_stream_row_bytes", [](int max_frames, int V, int beam_width, bool with_lm) {
    return e2e_asg_beam_stream_row_bytes(max_frames, V, beam_width, with_lm ? 1 : 0);
  });
  m.def("asg_beam_stream_workspace_bytes", [](int B, int V, int beam_width, bool with_lm) {
    return e2e_asg_beam_stream_workspace_bytes(B, V, beam_width, with_lm ? 1 : 0);
  });

  m.def("asg_beam_stream",
        [](uintptr_t x, int dtype, int64_t sB, int64_t sT, int64_t sV, uintptr_t transitions, uintptr_t chunk_len, int B,
           int T, int V, int num_replabels, int beam_width, int space_id, uintptr_t lm, double lmwt, double wip,
           double oov_penalty, uintptr_t state, size_t row_bytes, int max_frames, int nbest, uintptr_t out,
           int64_t max_out, uintptr_t out_len, uintptr_t n_hyp, uintptr_t scores, uintptr_t counts, uintptr_t frames_done,
           uintptr_t workspace, size_t workspace_bytes, uintptr_t stream, bool restrict_to_lexicon, uintptr_t timesteps) {
          e2e_asg_beam_opts o{restrict_to_lexicon ? 1 : 0, ptr<int64_t>(timesteps)};
          check(e2e_asg_beam_stream(ptr<const void>(x), dtype, sB, sT, sV, ptr<const void>(transitions),
                                    ptr<const int64_t>(chunk_len), B, T, V, num_replabels, beam_width, space_id,
                                    ptr<const e2e_lm>(lm), lmwt, wip, oov_penalty, ptr<void>(state), row_bytes, max_frames,
                                    nbest, ptr<int64_t>(out), max_out, ptr<int64_t>(out_len), ptr<int64_t>(n_hyp),
                                    ptr<double>(scores), ptr<int32_t>(counts), ptr<int64_t>(frames_done),
                                    ptr<void>(workspace), workspace_bytes, ptr<void>(stream), &o));
        },
        py::arg("x"), py::arg("dtype"), py::arg("sB"), py::arg("sT"), py::arg("sV"), py::arg("transitions"),
        py::arg("chunk_len"), py::arg("B"), py::arg("T"), py::arg("V"), py::arg("num_replabels"), py::arg("beam_width"),
        py::arg("space_id"), py::arg("lm"), py::arg("lmwt"), py::arg("wip"), py::arg("oov_penalty"), py::arg("state"),
        py::arg("row_bytes"), py::arg("max_frames"), py::arg("nbest"), py::arg("out"), py::arg("max_out"),
        py::arg("out_len"), py::arg("n_hyp"), py::arg("scores"), py::arg("counts"), py::arg("frames_done"),
        py::arg("workspace"), py::arg("workspace_bytes"), py::arg("stream"), py::arg("restrict_to_lexicon") = false,
        py::arg("timesteps") = (uintptr_t)0);

  m.def("ctc_scale_grads",
        [](uintptr_t grads, int dtype, uintptr_t scale, int B, int64_t row_elems, uintptr_t stream) {
          check(e2e_ctc_scale_grads(ptr<void>(grads), dtype, ptr<const void>(scale), B, row_elems, ptr<void>(stream)));
        },
        py::arg("grads"), py::arg("dtype"), py::arg("scale"), py::arg("B"), py::arg("row_elems"), py::arg("stream"));

  m.def("ctc_greedy",
        [](uintptr_t x, int dtype, int64_t sB, int64_t sT, int64_t sV, uintptr_t x_len, int B, int T, int V, int blank,
           uintptr_t out, uintptr_t out_len, uintptr_t stream) {
          check(e2e_ctc_greedy(ptr<const void>(x), dtype, sB, sT, sV, ptr<const int64_t>(x_len), B, T, V, blank,
                               ptr<int64_t>(out), ptr<int64_t>(out_len), ptr<void>(stream)));
        },
        py::arg("x"), py::arg("dtype"), py::arg("sB"), py::arg("sT"), py::arg("sV"), py::arg("x_len"), py::arg("B"),
        py::arg("T"), py::arg("V"), py::arg("blank"), py::arg("out"), py::arg("out_len"), py::arg("stream"));

  m.def("ctc_beam_workspace_bytes",
        [](int B, int T, int V, int beam_width) { return e2e_ctc_beam_workspace_bytes(B, T, V, beam_width); });
  m.def("ctc_beam_workspace_bytes_lm", [](int B, int T, int V, int beam_width, bool with_lm) {
    return e2e_ctc_beam_workspace_bytes_lm(B, T, V, beam_width, with_lm ? 1 : 0);
  });

  m.def("ctc_beam_max_width", [](int V, bool with_lm) { return e2e_ctc_beam_max_width(V, with_lm ? 1 : 0); });

  m.def("ctc_beam",
        [](uintptr_t lp, int dtype, int64_t sB, int64_t sT, int64_t sV, uintptr_t x_len, int B, int T, int V, int blank,
           int beam_width, int space_id, uintptr_t lm, double lmwt, double wip, double oov_penalty, uintptr_t out,
           int64_t max_out, uintptr_t out_len, uintptr_t workspace, size_t workspace_bytes, uintptr_t stream) {
          check(e2e_ctc_beam(ptr<const void>(lp), dtype, sB, sT, sV, ptr<const int64_t>(x_len), B, T, V, blank,
                             beam_width, space_id, ptr<const e2e_lm>(lm), lmwt, wip, oov_penalty, ptr<int64_t>(out),
                             max_out, ptr<int64_t>(out_len), ptr<void>(workspace), workspace_bytes, ptr<void>(stream)));
        },
        py::arg("lp"), py::arg("dtype"), py::arg("sB"), py::arg("sT"), py::arg("sV"), py::arg("x_len"), py::arg("B"),
        py::arg("T"), py::arg("V"), py::arg("blank"), py::arg("beam_width"), py::arg("space_id"), py::arg("lm"),
        py::arg("lmwt"), py::arg("wip"), py::arg("oov_penalty"), py::arg("out"), py::arg("max_out"),
        py::arg("out_len"), py::arg("workspace"), py::arg("workspace_bytes"), py::arg("stream"));

  m.def("ctc_beam_nbest_workspace_bytes", [](int B, int T, int V, int beam_width, bool with_lm, bool with_timesteps) {
    return e2e_ctc_beam_nbest_workspace_bytes(B, T, V, beam_width, with_lm ? 1 : 0, with_timesteps ? 1 : 0);
  });

  m.def("ctc_beam_nbest",
        [](uintptr_t lp, int dtype, int64_t sB, int64_t sT, int64_t sV, uintptr_t x_len, int B, int T, int V, int blank,
           int beam_width, int space_id, uintptr_t lm, double lmwt, double wip, double oov_penalty, int nbest,
           uintptr_t out, int64_t max_out, uintptr_t out_len, uintptr_t n_hyp, uintptr_t scores, uintptr_t counts,
           uintptr_t timesteps, uintptr_t workspace, size_t workspace_bytes, uintptr_t stream, bool restrict_to_lexicon) {
          e2e_ctc_beam_opts o{restrict_to_lexicon ? 1 : 0};
          check(e2e_ctc_beam_nbest_opt(ptr<const void>(lp), dtype, sB, sT, sV, ptr<const int64_t>(x_len), B, T, V, blank,
                                       beam_width, space_id, ptr<const e2e_lm>(lm), lmwt, wip, oov_penalty, nbest,
                                       ptr<int64_t>(out), max_out, ptr<int64_t>(out_len), ptr<int64_t>(n_hyp),
                                       ptr<double>(scores), ptr<int32_t>(counts), ptr<int64_t>(timesteps),
                                       ptr<void>(workspace), workspace_bytes, ptr<void>(stream), &o));
        },
        py::arg("lp"), py::arg("dtype"), py::arg("sB"), py::arg("sT"), py::arg("sV"), py::arg("x_len"), py::arg("B"),
        py::arg("T"), py::arg("V"), py::arg("blank"), py::arg("beam_width"), py::arg("space_id"), py::arg("lm"),
        py::arg("lmwt"), py::arg("wip"), py::arg("oov_penalty"), py::arg("nbest"), py::arg("out"), py::arg("max_out"),
        py::arg("out_len"), py::arg("n_hyp"), py::arg("scores"), py::arg("counts"), py::arg("timesteps"),
        py::arg("workspace"), py::arg("workspace_bytes"), py::arg("stream"), py::arg("restrict_to_lexicon") = false);

  m.def("ctc_beam_stream_row_bytes", [](int max_frames, int V, int beam_width, bool with_lm, bool with_timesteps) {
    return e2e_ctc_beam_stream_row_bytes(max_frames, V, beam_width, with_lm ? 1 : 0, with_timesteps ? 1 : 0);
  });
  m.def("ctc_beam_stream_workspace_bytes", [](int B, int V, int beam_width, bool with_lm) {
    return e2e_ctc_beam_stream_workspace_bytes(B, V, beam_width, with_lm ? 1 : 0);
  });

  m.def("ctc_beam_stream",
        [](uintptr_t lp, int dtype, int64_t sB, int64_t sT, int64_t sV, uintptr_t chunk_len, int B, int T, int V, int blank,
           int beam_width, int space_id, uintptr_t lm, double lmwt, double wip, double oov_penalty, uintptr_t state,
           size_t row_bytes, int max_frames, bool with_timesteps, int nbest, uintptr_t out, int64_t max_out,
           uintptr_t out_len, uintptr_t n_hyp, uintptr_t scores, uintptr_t counts, uintptr_t timesteps,
           uintptr_t frames_done, uintptr_t workspace, size_t workspace_bytes, uintptr_t stream, bool restrict_to_lexicon) {
          e2e_ctc_beam_opts o{restrict_to_lexicon ? 1 : 0};
          check(e2e_ctc_beam_stream(ptr<const void>(lp), dtype, sB, sT, sV, ptr<const int64_t>(chunk_len), B, T, V, blank,
                                    beam_width, space_id, ptr<const e2e_lm>(lm), lmwt, wip, oov_penalty, ptr<void>(state),
                                    row_bytes, max_frames, with_timesteps ? 1 : 0, nbest, ptr<int64_t>(out), max_out,
                                    ptr<int64_t>(out_len), ptr<int64_t>(n_hyp), ptr<double>(scores), ptr<int32_t>(counts),
                                    ptr<int64_t>(timesteps), ptr<int64_t>(frames_done), ptr<void>(workspace),
                                    workspace_bytes, ptr<void>(stream), &o));
        },
        py::arg("lp"), py::arg("dtype"), py::arg("sB"), py::arg("sT"), py::arg("sV"), py::arg("chunk_len"), py::arg("B"),
        py::arg("T"), py::arg("V"), py::arg("blank"), py::arg("beam_width"), py::arg("space_id"), py::arg("lm"),
        py::arg("lmwt"), py::arg("wip"), py::arg("oov_penalty"), py::arg("state"), py::arg("row_bytes"),
        py::arg("max_frames"), py::arg("with_timesteps"), py::arg("nbest"), py::arg("out"), py::arg("max_out"),
        py::arg("out_len"), py::arg("n_hyp"), py::arg("scores"), py::arg("counts"), py::arg("timesteps"),
        py::arg("frames_done"), py::arg("workspace"), py::arg("workspace_bytes"), py::arg("stream"),
        py::arg("restrict_to_lexicon") = false);

  // per-frame label pruning: the selection alone, and the pruned searches (cutoff_top_n, cutoff_prob behind the unpruned
  // calls' arguments)
  m.def("ctc_label_cut_max", [] { return e2e_ctc_label_cut_max(); });
  m.def("ctc_label_cut_workspace_bytes",
        [](int B, int T, int V, int cutoff_top_n) { return e2e_ctc_label_cut_workspace_bytes(B, T, V, cutoff_top_n); });
  m.def("ctc_label_cut",
        [](uintptr_t lp, int dtype, int64_t sB, int64_t sT, int64_t sV, uintptr_t x_len, int B, int T, int V, int blank,
           int cutoff_top_n, double cutoff_prob, uintptr_t ids, uintptr_t n, uintptr_t workspace, size_t workspace_bytes,
           uintptr_t stream) {
          check(e2e_ctc_label_cut(ptr<const void>(lp), dtype, sB, sT, sV, ptr<const int64_t>(x_len), B, T, V, blank,
                                  cutoff_top_n, cutoff_prob, ptr<int32_t>(ids), ptr<int32_t>(n), ptr<void>(workspace),
                                  workspace_bytes, ptr<void>(stream)));
        },
        py::arg("lp"), py::arg("dtype"), py::arg("sB"), py::arg("sT"), py::arg("sV"), py::arg("x_len"), py::arg("B"),
        py::arg("T"), py::arg("V"), py::arg("blank"), py::arg("cutoff_top_n"), py::arg("cutoff_prob"), py::arg("ids"),
        py::arg("n"), py::arg("workspace"), py::arg("workspace_bytes"), py::arg("stream"));
  m.def("ctc_beam_cut_max_width", [](int V, bool with_lm) { return e2e_ctc_beam_cut_max_width(V, with_lm ? 1 : 0); });
  m.def("ctc_beam_cut_workspace_bytes",
        [](int B, int T, int V, int beam_width, bool with_lm, bool with_timesteps, int cutoff_top_n) {
          return e2e_ctc_beam_cut_workspace_bytes(B, T, V, beam_width, with_lm ? 1 : 0, with_timesteps ? 1 : 0, cutoff_top_n);
        });
  m.def("ctc_beam_cut_stream_workspace_bytes", [](int B, int T, int V, int beam_width, bool with_lm, int cutoff_top_n) {
    return e2e_ctc_beam_cut_stream_workspace_bytes(B, T, V, beam_width, with_lm ? 1 : 0, cutoff_top_n);
  });
  m.def("ctc_beam_nbest_cut",
        [](uintptr_t lp, int dtype, int64_t sB, int64_t sT, int64_t sV, uintptr_t x_len, int B, int T, int V, int blank,
           int beam_width, int space_id, uintptr_t lm, double lmwt, double wip, double oov_penalty, int nbest,
           uintptr_t out, int64_t max_out, uintptr_t out_len, uintptr_t n_hyp, uintptr_t scores, uintptr_t counts,
           uintptr_t timesteps, uintptr_t workspace, size_t workspace_bytes, uintptr_t stream, bool restrict_to_lexicon,
           int cutoff_top_n, double cutoff_prob) {
          e2e_ctc_beam_opts o{restrict_to_lexicon ? 1 : 0};
          check(e2e_ctc_beam_nbest_cut(ptr<const void>(lp), dtype, sB, sT, sV, ptr<const int64_t>(x_len), B, T, V, blank,
                                       beam_width, space_id, ptr<const e2e_lm>(lm), lmwt, wip, oov_penalty, nbest,
                                       ptr<int64_t>(out), max_out, ptr<int64_t>(out_len), ptr<int64_t>(n_hyp),
                                       ptr<double>(scores), ptr<int32_t>(counts), ptr<int64_t>(timesteps),
                                       ptr<void>(workspace), workspace_bytes, ptr<void>(stream), &o, cutoff_top_n, cutoff_prob));
        },
        py::arg("lp"), py::arg("dtype"), py::arg("sB"), py::arg("sT"), py::arg("sV"), py::arg("x_len"), py::arg("B"),
        py::arg("T"), py::arg("V"), py::arg("blank"), py::arg("beam_width"), py::arg("space_id"), py::arg("lm"),
        py::arg("lmwt"), py::arg("wip"), py::arg("oov_penalty"), py::arg("nbest"), py::arg("out"), py::arg("max_out"),
        py::arg("out_len"), py::arg("n_hyp"), py::arg("scores"), py::arg("counts"), py::arg("timesteps"),
        py::arg("workspace"), py::arg("workspace_bytes"), py::arg("stream"), py::arg("restrict_to_lexicon"),
        py::arg("cutoff_top_n"), py::arg("cutoff_prob"));
  m.def("ctc_beam_stream_cut",
        [](uintptr_t lp, int dtype, int64_t sB, int64_t sT, int64_t sV, uintptr_t chunk_len, int B, int T, int V, int blank,
           int beam_width, int space_id, uintptr_t lm, double lmwt, double wip, double oov_penalty, uintptr_t state,
           size_t row_bytes, int max_frames, bool with_timesteps, int nbest, uintptr_t out, int64_t max_out,
           uintptr_t out_len, uintptr_t n_hyp, uintptr_t scores, uintptr_t counts, uintptr_t timesteps,
           uintptr_t frames_done, uintptr_t workspace, size_t workspace_bytes, uintptr_t stream, bool restrict_to_lexicon,
           int cutoff_top_n, double cutoff_prob) {
          e2e_ctc_beam_opts o{restrict_to_lexicon ? 1 : 0};
          check(e2e_ctc_beam_stream_cut(ptr<const void>(lp), dtype, sB, sT, sV, ptr<const int64_t>(chunk_len), B, T, V, blank,
                                        beam_width, space_id, ptr<const e2e_lm>(lm), lmwt, wip, oov_penalty, ptr<void>(state),
                                        row_bytes, max_frames, with_timesteps ? 1 : 0, nbest, ptr<int64_t>(out), max_out,
                                        ptr<int64_t>(out_len), ptr<int64_t>(n_hyp), ptr<double>(scores), ptr<int32_t>(counts),
                                        ptr<int64_t>(timesteps), ptr<int64_t>(frames_done), ptr<void>(workspace),
                                        workspace_bytes, ptr<void>(stream), &o, cutoff_top_n, cutoff_prob));
        },
        py::arg("lp"), py::arg("dtype"), py::arg("sB"), py::arg("sT"), py::arg("sV"), py::arg("chunk_len"), py::arg("B"),
        py::arg("T"), py::arg("V"), py::arg("blank"), py::arg("beam_width"), py::arg("space_id"), py::arg("lm"),
        py::arg("lmwt"), py::arg("wip"), py::arg("oov_penalty"), py::arg("state"), py::arg("row_bytes"),
        py::arg("max_frames"), py::arg("with_timesteps"), py::arg("nbest"), py::arg("out"), py::arg("max_out"),
        py::arg("out_len"), py::arg("n_hyp"), py::arg("scores"), py::arg("counts"), py::arg("timesteps"),
        py::arg("frames_done"), py::arg("workspace"), py::arg("workspace_bytes"), py::arg("stream"),
        py::arg("restrict_to_lexicon"), py::arg("cutoff_top_n"), py::arg("cutoff_prob"));

  m.def("ctc_align_workspace_bytes",
        [](int B, int T, int V, int Smax, bool is_ctc) { return e2e_ctc_align_workspace_bytes(B, T, V, Smax, is_ctc ? 1 : 0); });

  m.def("ctc_align",
        [](uintptr_t lp, int dtype, int64_t sB, int64_t sT, int64_t sV, uintptr_t targets, int64_t tgt_stride,
           uintptr_t x_len, uintptr_t t_len, int B, int T, int V, int Smax, int blank, bool is_ctc, uintptr_t out,
           int64_t pad_value, uintptr_t workspace, size_t workspace_bytes, uintptr_t stream) {
          check(e2e_ctc_align(ptr<const void>(lp), dtype, sB, sT, sV, ptr<const int64_t>(targets), tgt_stride,
                              ptr<const int64_t>(x_len), ptr<const int64_t>(t_len), B, T, V, Smax, blank,
                              is_ctc ? 1 : 0, ptr<int64_t>(out), pad_value, ptr<void>(workspace), workspace_bytes,
                              ptr<void>(stream)));
        },
        py::arg("lp"), py::arg("dtype"), py::arg("sB"), py::arg("sT"), py::arg("sV"), py::arg("targets"),
        py::arg("tgt_stride"), py::arg("x_len"), py::arg("t_len"), py::arg("B"), py::arg("T"), py::arg("V"),
        py::arg("Smax"), py::arg("blank"), py::arg("is_ctc"), py::arg("out"), py::arg("pad_value"),
        py::arg("workspace"), py::arg("workspace_bytes"), py::arg("stream"));

  m.attr("WORDSEG_HEADER") = E2E_WORDSEG_HEADER;
  m.attr("WORDSEG_WHOLE") = E2E_WORDSEG_WHOLE;
  m.attr("WORDSEG_FRAME") = E2E_WORDSEG_FRAME;
  m.attr("WORDSEG_CHUNK") = E2E_WORDSEG_CHUNK;
  m.def("ctc_wordseg_table_elems", [](int B, int T) { return e2e_ctc_wordseg_table_elems(B, T); });
  m.def("ctc_wordseg_workspace_bytes", [](int B, int T) { return e2e_ctc_wordseg_workspace_bytes(B, T); });

  m.def("ctc_wordseg_plan",
        [](uintptr_t x, int dtype, int64_t sB, int64_t sT, int64_t sV, uintptr_t align, uintptr_t targets,
           int64_t tgt_stride, uintptr_t x_len, uintptr_t t_len, int B, int T, int V, int Smax, int blank, int space,
           int min_word_length, uintptr_t table, size_t table_elems, uintptr_t pool, uintptr_t workspace,
           size_t workspace_bytes, uintptr_t stream) {
          check(e2e_ctc_wordseg_plan(ptr<const void>(x), dtype, sB, sT, sV, ptr<const int64_t>(align),
                                     ptr<const int64_t>(targets), tgt_stride, ptr<const int64_t>(x_len),
                                     ptr<const int64_t>(t_len), B, T, V, Smax, blank, space, min_word_length,
                                     ptr<int32_t>(table), table_elems, ptr<int64_t>(pool), ptr<void>(workspace),
                                     workspace_bytes, ptr<void>(stream)));
        },
        py::arg("x"), py::arg("dtype"), py::arg("sB"), py::arg("sT"), py::arg("sV"), py::arg("align"), py::arg("targets"),
        py::arg("tgt_stride"), py::arg("x_len"), py::arg("t_len"), py::arg("B"), py::arg("T"), py::arg("V"),
        py::arg("Smax"), py::arg("blank"), py::arg("space"), py::arg("min_word_length"), py::arg("table"),
        py::arg("table_elems"), py::arg("pool"), py::arg("workspace"), py::arg("workspace_bytes"), py::arg("stream"));

  m.def("ctc_wordseg_gather",
        [](uintptr_t x, int dtype, int64_t sB, int64_t sT, int64_t sV, uintptr_t targets, int64_t tgt_stride,
           uintptr_t x_len, uintptr_t t_len, int B, int T, int V, int Smax, uintptr_t table, uintptr_t pool,
           uintptr_t idx, int n_idx, int L, int S, uintptr_t xg, uintptr_t tg, uintptr_t xlg, uintptr_t tlg,
           uintptr_t stream) {
          check(e2e_ctc_wordseg_gather(ptr<const void>(x), dtype, sB, sT, sV, ptr<const int64_t>(targets), tgt_stride,
                                       ptr<const int64_t>(x_len), ptr<const int64_t>(t_len), B, T, V, Smax,
                                       ptr<const int32_t>(table), ptr<const int64_t>(pool), ptr<const int32_t>(idx),
                                       n_idx, L, S, ptr<void>(xg), ptr<int64_t>(tg), ptr<int64_t>(xlg),
                                       ptr<int64_t>(tlg), ptr<void>(stream)));
        },
        py::arg("x"), py::arg("dtype"), py::arg("sB"), py::arg("sT"), py::arg("sV"), py::arg("targets"),
        py::arg("tgt_stride"), py::arg("x_len"), py::arg("t_len"), py::arg("B"), py::arg("T"), py::arg("V"),
        py::arg("Smax"), py::arg("table"), py::arg("pool"), py::arg("idx"), py::arg("n_idx"), py::arg("L"), py::arg("S"),
        py::arg("xg"), py::arg("tg"), py::arg("xlg"), py::arg("tlg"), py::arg("stream"));

  m.def("ctc_wordseg_finish",
        [](uintptr_t x, int dtype, int64_t sB, int64_t sT, int64_t sV, uintptr_t align, int B, int T, int V,
           uintptr_t table, uintptr_t g_grads, uintptr_t g_losses, uintptr_t g_idx, int n_idx, int L, bool last,
           uintptr_t losses, uintptr_t grads, uintptr_t workspace, size_t workspace_bytes, uintptr_t stream) {
          check(e2e_ctc_wordseg_finish(ptr<const void>(x), dtype, sB, sT, sV, ptr<const int64_t>(align), B, T, V,
                                       ptr<const int32_t>(table), ptr<const void>(g_grads), ptr<const void>(g_losses),
                                       ptr<const int32_t>(g_idx), n_idx, L, last ? 1 : 0, ptr<void>(losses),
                                       ptr<void>(grads), ptr<void>(workspace), workspace_bytes, ptr<void>(stream)));
        },
        py::arg("x"), py::arg("dtype"), py::arg("sB"), py::arg("sT"), py::arg("sV"), py::arg("align"), py::arg("B"),
        py::arg("T"), py::arg("V"), py::arg("table"), py::arg("g_grads"), py::arg("g_losses"), py::arg("g_idx"),
        py::arg("n_idx"), py::arg("L"), py::arg("last"), py::arg("losses"), py::arg("grads"), py::arg("workspace"),
        py::arg("workspace_bytes"), py::arg("stream"));

  py::class_<LanguageModel>(m, "LanguageModel")
      .def(py::init<const std::string&, const std::vector<std::string>&, bool>(), py::arg("path"), py::arg("labels"),
           py::arg("case_sensitive"))
      .def_static("from_words",
                  [](const std::vector<std::string>& words, const std::vector<std::string>& labels, bool case_sensitive) {
                    return new LanguageModel(LanguageModel::FromWords{}, words, labels, case_sensitive);
                  },
                  py::arg("words"), py::arg("labels"), py::arg("case_sensitive"), py::return_value_policy::take_ownership)
      .def_static("from_transcriptions",
                  [](const std::string& path, const std::vector<std::string>& words, const std::vector<int32_t>& label_ids,
                     const std::vector<int32_t>& offsets, const std::vector<std::string>& labels, bool case_sensitive) {
                    return new LanguageModel(LanguageModel::FromTranscriptions{}, path, words, label_ids, offsets, labels,
                                             case_sensitive);
                  },
                  py::arg("path"), py::arg("words"), py::arg("label_ids"), py::arg("offsets"), py::arg("labels"),
                  py::arg("case_sensitive"), py::return_value_policy::take_ownership)
      .def("is_transcribed", &LanguageModel::is_transcribed)
      .def("transcriptions_dropped", &LanguageModel::transcriptions_dropped)
      .def("transcribe", &LanguageModel::transcribe, py::arg("ids"), py::arg("space_id"))
      .def("word_string", &LanguageModel::word_string, py::arg("id"))
      .def_property_readonly("handle", &LanguageModel::handle)
      .def("enable_lexicon", &LanguageModel::enable_lexicon)
      .def("has_lexicon", &LanguageModel::has_lexicon)
      .def("spelling_class", &LanguageModel::spelling_class, py::arg("spelling"))
      .def("order", &LanguageModel::order)
      .def("device", &LanguageModel::device)
      .def("word_index", &LanguageModel::word_index, py::arg("word"))
      .def("score", &LanguageModel::score, py::arg("ctx"), py::arg("word"));
}
