// end2end_amd._C -- the thin pybind11 layer between the Python host code and the C ABI of libe2e_ctc.so
// (include/e2e_ctc.h).  It stands where the reference's pybind modules stand (src/losses/ctc_loss_py.cpp:5-17,
// src/decoders/ctc_decoder_py.cpp:5-39) but carries no tensor types: the Python side hands device addresses
// (tensor.data_ptr()), strides and sizes; every function forwards to exactly one extern "C" entry point and turns a
// negative return code into the Python exception E2EError carrying e2e_last_error().
//
// The header's parameter lists are not written out again here: a wrapper's Python signature and its forwarding call are
// deduced from the entry point's own type (Binder, below), and an entry gives only its argument names -- all but the three
// loss calls that check their arguments first, which are lambdas and name each argument once more.  The same deduction
// fills _C.SIGNATURES, from which end2end_amd/_lib.py types the ctypes view of the library.
//
// Compiled with plain g++ against the pybind11 headers (no torch headers, no HIP headers): end2end_amd/csrc/Makefile.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstdint>
#include <optional>
#include <sstream>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../../include/e2e_ctc.h"
#include "../../../include/e2e_ctc_debug.h"

namespace py = pybind11;

namespace {

struct E2EError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

inline void check(int rc) {
  if (rc != E2E_OK) throw E2EError(std::string("libe2e_ctc: ") + e2e_last_error() + " (code " + std::to_string(rc) + ")");
}

// ---- a C parameter as Python sees it: a pointer travels as an integer (data_ptr(), a stream, a model's handle), every
// other type as itself ----
template <typename T>
using py_t = std::conditional_t<std::is_pointer_v<T>, uintptr_t, T>;

template <typename T, typename V>
inline T to_c(V v) {
  if constexpr (std::is_pointer_v<T> && !std::is_pointer_v<V>) return reinterpret_cast<T>(static_cast<uintptr_t>(v));
  else return v;
}

// fn(v...), every integer that stands for a pointer turned into that pointer: for the wrappers that are written out
template <typename R, typename... A, typename... V>
inline R forward(R (*fn)(A...), V... v) { return fn(to_c<A>(v)...); }

// ---- one character per type, for SIGNATURES.  Lower case: values; upper case: the pointer to that value type ----
template <typename T>
constexpr char type_code() {
  if constexpr (std::is_pointer_v<T>) {
    using E = std::remove_cv_t<std::remove_pointer_t<T>>;
    if constexpr (std::is_void_v<E>) return 'p';
    else if constexpr (std::is_same_v<E, char>) return 's';
    else if constexpr (std::is_same_v<E, const char*>) return 'S';
    else if constexpr (std::is_same_v<E, e2e_lm>) return 'm';
    else if constexpr (std::is_same_v<E, e2e_lm*>) return 'M';
    else if constexpr (std::is_same_v<E, e2e_ctc_loss_opts>) return 'O';
    else if constexpr (std::is_same_v<E, e2e_ctc_beam_opts>) return 'C';
    else if constexpr (std::is_same_v<E, e2e_asg_beam_opts>) return 'A';
    else if constexpr (std::is_same_v<E, e2e_gram_beam_opts>) return 'G';
    else return type_code<E>() - 'a' + 'A';                    // I, Q, U, D
  } else {
    static_assert(std::is_void_v<T> || std::is_same_v<T, int> || std::is_same_v<T, int64_t> || std::is_same_v<T, size_t> ||
                      std::is_same_v<T, double> || std::is_same_v<T, uint32_t> || std::is_same_v<T, long long>,
                  "a type the C ABI has not used yet: give it a code here and a ctypes type in end2end_amd/_lib.py");
    return std::is_void_v<T> ? 'v' : std::is_same_v<T, int> ? 'i' : std::is_same_v<T, int64_t> ? 'q'
         : std::is_same_v<T, size_t> ? 'z' : std::is_same_v<T, double> ? 'd' : std::is_same_v<T, uint32_t> ? 'u' : 'l';
  }
}

template <typename R, typename... A>
std::string signature(R (*)(A...)) { return std::string{type_code<R>(), ':', type_code<A>()...}; }

// ---- the wrapper of an entry point whose Python arguments are its C parameters, one to one ----
template <auto Fn, bool Checked, typename = decltype(Fn)>
struct direct;
template <auto Fn, bool Checked, typename R, typename... A>
struct direct<Fn, Checked, R (*)(A...)> {
  auto operator()(py_t<A>... a) const {
    if constexpr (Checked) check(Fn(to_c<A>(a)...));
    else return Fn(to_c<A>(a)...);
  }
};

// ---- the wrapper of an entry point whose options struct is spread into Python arguments: Python passes Make's parameters
// where C takes `const O*`, everything before and after it one to one.  Make gives the struct, or nothing for NULL ----
template <auto Fn, auto Make, typename = decltype(Fn), typename = decltype(Make)>
struct spread;
template <auto Fn, auto Make, typename... A, typename O, typename... E>
struct spread<Fn, Make, int (*)(A...), std::optional<O> (*)(E...)> {
  using Args = std::tuple<A...>;
  static constexpr size_t at() {
    size_t i = 0;
    (void)((std::is_same_v<A, const O*> || (++i, false)) || ...);
    return i;
  }
  static_assert(at() < sizeof...(A), "the entry point does not take these options");
  template <size_t... H, size_t... T>
  static auto wrapper(std::index_sequence<H...>, std::index_sequence<T...>) {
    return [](py_t<std::tuple_element_t<H, Args>>... head, E... e, py_t<std::tuple_element_t<at() + 1 + T, Args>>... tail) {
      std::optional<O> o = Make(e...);
      check(Fn(to_c<std::tuple_element_t<H, Args>>(head)..., o ? &*o : nullptr,
               to_c<std::tuple_element_t<at() + 1 + T, Args>>(tail)...));
    };
  }
  static auto fn() { return wrapper(std::make_index_sequence<at()>{}, std::make_index_sequence<sizeof...(A) - at() - 1>{}); }
};

std::optional<e2e_ctc_loss_opts> loss_opts(double grad_scale, uintptr_t reduced, int reduction, int chains) {
  return e2e_ctc_loss_opts{grad_scale, to_c<void*>(reduced), reduction, chains};
}
std::optional<e2e_ctc_beam_opts> ctc_beam_opts(bool restrict_to_lexicon) { return e2e_ctc_beam_opts{restrict_to_lexicon ? 1 : 0}; }
std::optional<e2e_asg_beam_opts> asg_beam_opts(bool restrict_to_lexicon, uintptr_t timesteps) {
  return e2e_asg_beam_opts{restrict_to_lexicon ? 1 : 0, to_c<int64_t*>(timesteps)};
}
// opts: None passes NULL; else (restrict_to_lexicon, timesteps) -- zeros included, to tell the two apart
std::optional<e2e_gram_beam_opts> gram_beam_opts(py::object opts) {
  if (opts.is_none()) return std::nullopt;
  auto t = opts.cast<std::pair<bool, uintptr_t>>();
  return e2e_gram_beam_opts{t.first ? 1 : 0, to_c<int64_t*>(t.second)};
}

template <typename F>
struct arity : arity<decltype(&F::operator())> {};
template <typename R, typename... A>
struct arity<R (*)(A...)> : std::integral_constant<size_t, sizeof...(A)> {};
template <typename C, typename R, typename... A>
struct arity<R (C::*)(A...) const> : std::integral_constant<size_t, sizeof...(A)> {};

// ---- what an entry of the module's table says: the C function, its name, and the Python names of the arguments ----
struct Binder {
  py::module_& m;
  py::dict sigs;

  // the signature alone: a symbol of the headers that no function of this module forwards to one to one
  template <auto Fn>
  void sig(const char* cname) { sigs[cname] = signature(Fn); }

  // an entry point that returns a code: e2e_<name> becomes <name>(names...) -> None, raising E2EError
  template <auto Fn>
  void call(const char* cname, const char* names) { sig<Fn>(cname); def(cname + 4, names, direct<Fn, true>{}); }

  // a query (*_bytes, *_max*, takes_dtype): e2e_<name> becomes <name>(positional arguments) -> its value
  template <auto Fn>
  void query(const char* cname) { sig<Fn>(cname); m.def(cname + 4, direct<Fn, false>{}); }

  // an entry point whose options struct Python passes spread out (spread and the makers above): it becomes `name`
  template <auto Fn, auto Make, typename... D>
  void call_opts(const char* cname, const char* name, const char* names, D... defaults) {
    sig<Fn>(cname);
    def(name, names, spread<Fn, Make>::fn(), defaults...);
  }

  // f under `name` with the blank-separated `names`, the last of them with `defaults`.  One name per argument: a count
  // that differs from f's arity fails the import.
  template <typename F, typename... D>
  void def(const char* name, const char* names, F f, D... defaults) {
    std::vector<std::string> n;
    std::istringstream in(names);
    for (std::string s; in >> s;) n.push_back(s);
    constexpr size_t N = arity<F>::value;
    static_assert(sizeof...(D) <= N);
    if (n.size() != N)
      throw std::runtime_error(std::string(name) + ": " + std::to_string(n.size()) + " argument names for " + std::to_string(N) +
                               " arguments");
    def_named(name, n, f, std::make_index_sequence<N - sizeof...(D)>{}, std::index_sequence_for<D...>{},
              std::make_tuple(defaults...));
  }
  template <typename F, size_t... I, size_t... J, typename T>
  void def_named(const char* name, const std::vector<std::string>& n, F f, std::index_sequence<I...>, std::index_sequence<J...>,
                 const T& defaults) {
    m.def(name, f, py::arg(n[I].c_str())..., (py::arg(n[sizeof...(I) + J].c_str()) = std::get<J>(defaults))...);
  }
};

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
  m.attr("WORDSEG_HEADER") = E2E_WORDSEG_HEADER;
  m.attr("WORDSEG_WHOLE") = E2E_WORDSEG_WHOLE;
  m.attr("WORDSEG_FRAME") = E2E_WORDSEG_FRAME;
  m.attr("WORDSEG_CHUNK") = E2E_WORDSEG_CHUNK;

  Binder b{m, py::dict()};
  // SIGNATURES: every function of the two headers -> "<return>:<parameters>", one character per type (type_code)
  m.attr("SIGNATURES") = b.sigs;

  b.sig<e2e_ctc_abi_version>("e2e_ctc_abi_version");
  m.def("abi_version", [] { return e2e_ctc_abi_version(); });
  b.sig<e2e_last_error>("e2e_last_error");
  m.def("last_error", [] { return std::string(e2e_last_error()); });

  // ---- the losses ----
  b.query<e2e_ctc_loss_workspace_bytes>("e2e_ctc_loss_workspace_bytes");
  b.query<e2e_ctc_loss_takes_dtype>("e2e_ctc_loss_takes_dtype");
  b.sig<e2e_ctc_loss_fwd_bwd>("e2e_ctc_loss_fwd_bwd");
  // (grad_scale / reduced / reduction / chains: e2e_ctc_loss_opts; the defaults are the plain call)
  b.call_opts<e2e_ctc_loss_fwd_bwd_opt, loss_opts>("e2e_ctc_loss_fwd_bwd_opt", "ctc_loss_fwd_bwd",
        "x dtype input_is_logprobs sB sT sV targets tgt_stride x_len t_len B T V Smax blank losses grads workspace "
        "workspace_bytes algo stream grad_scale reduced reduction chains", 1.0, 0, E2E_REDUCE_NONE, E2E_CHAINS_F64);
  b.call<e2e_ctc_scale_grads>("e2e_ctc_scale_grads", "grads dtype scale B row_elems stream");

  b.query<e2e_ctc_noblank_workspace_bytes>("e2e_ctc_noblank_workspace_bytes");
  b.sig<e2e_ctc_noblank_fwd_bwd>("e2e_ctc_noblank_fwd_bwd");
  // (arguments the library would refuse are refused here too, before anything reaches the GPU)
  b.def("ctc_noblank_fwd_bwd",
        "x dtype input_is_logprobs sB sT sV targets tgt_stride x_len t_len B T V Smax space_idx losses grads workspace "
        "workspace_bytes stream grad_scale reduced reduction",
        [](uintptr_t x, int dtype, int input_is_logprobs, int64_t sB, int64_t sT, int64_t sV, uintptr_t targets,
           int64_t tgt_stride, uintptr_t x_len, uintptr_t t_len, int B, int T, int V, int Smax, int space_idx,
           uintptr_t losses, uintptr_t grads, uintptr_t workspace, size_t workspace_bytes, uintptr_t stream,
           double grad_scale, uintptr_t reduced, int reduction) {
          if (dtype != E2E_F32 && dtype != E2E_F64) throw py::value_error("ctc_noblank_fwd_bwd: dtype must be F32 or F64");
          if (V < 1 || (space_idx != -1 && (space_idx < 0 || space_idx >= V)))
            throw py::value_error("ctc_noblank_fwd_bwd: space_idx " + std::to_string(space_idx) + " is neither -1 nor in [0, " +
                                  std::to_string(V) + ")");
          if (reduction < E2E_REDUCE_NONE || reduction > E2E_REDUCE_MEAN || (reduction != E2E_REDUCE_NONE && !reduced))
            throw py::value_error("ctc_noblank_fwd_bwd: bad reduction");
          e2e_ctc_loss_opts o{grad_scale, to_c<void*>(reduced), reduction, E2E_CHAINS_F64};
          check(forward(e2e_ctc_noblank_fwd_bwd, x, dtype, input_is_logprobs, sB, sT, sV, targets, tgt_stride, x_len, t_len, B, T,
                        V, Smax, space_idx, losses, grads, workspace, workspace_bytes, stream, &o));
        },
        1.0, 0, E2E_REDUCE_NONE);

  b.query<e2e_gram_ctc_workspace_bytes>("e2e_gram_ctc_workspace_bytes");
  b.sig<e2e_gram_ctc_fwd_bwd>("e2e_gram_ctc_fwd_bwd");
  b.def("gram_ctc_fwd_bwd",
        "x dtype input_is_logprobs sB sT sV targets tgt_stride x_len t_len B T V Smax keys cols n_grams radix max_order losses "
        "grads workspace workspace_bytes stream grad_scale reduced reduction",
        [](uintptr_t x, int dtype, int input_is_logprobs, int64_t sB, int64_t sT, int64_t sV, uintptr_t targets,
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
          e2e_ctc_loss_opts o{grad_scale, to_c<void*>(reduced), reduction, E2E_CHAINS_F64};
          check(forward(e2e_gram_ctc_fwd_bwd, x, dtype, input_is_logprobs, sB, sT, sV, targets, tgt_stride, x_len, t_len, B, T, V,
                        Smax, keys, cols, n_grams, radix, max_order, losses, grads, workspace, workspace_bytes, stream, &o));
        },
        1.0, 0, E2E_REDUCE_NONE);

  b.query<e2e_asg_max_labels>("e2e_asg_max_labels");
  b.query<e2e_asg_max_target_length>("e2e_asg_max_target_length");
  b.query<e2e_asg_workspace_bytes>("e2e_asg_workspace_bytes");
  b.sig<e2e_asg_fwd_bwd>("e2e_asg_fwd_bwd");
  b.def("asg_fwd_bwd",
        "x dtype sB sT sV transitions targets tgt_stride x_len t_len B T V Smax losses grads tgrads workspace workspace_bytes "
        "stream grad_scale",
        [](uintptr_t x, int dtype, int64_t sB, int64_t sT, int64_t sV, uintptr_t transitions, uintptr_t targets,
           int64_t tgt_stride, uintptr_t x_len, uintptr_t t_len, int B, int T, int V, int Smax, uintptr_t losses,
           uintptr_t grads, uintptr_t tgrads, uintptr_t workspace, size_t workspace_bytes, uintptr_t stream,
           double grad_scale) {
          if (dtype != E2E_F32 && dtype != E2E_F64) throw py::value_error("asg_fwd_bwd: dtype must be F32 or F64");
          e2e_ctc_loss_opts o{grad_scale, nullptr, E2E_REDUCE_NONE, E2E_CHAINS_F64};
          check(forward(e2e_asg_fwd_bwd, x, dtype, sB, sT, sV, transitions, targets, tgt_stride, x_len, t_len, B, T, V, Smax,
                        losses, grads, tgrads, workspace, workspace_bytes, stream, &o));
        },
        1.0);
  b.query<e2e_asg_viterbi_workspace_bytes>("e2e_asg_viterbi_workspace_bytes");
  b.call<e2e_asg_viterbi>("e2e_asg_viterbi",
                          "x dtype sB sT sV transitions x_len B T V path pad_value scores collapsed lengths workspace "
                          "workspace_bytes stream");

  // ---- Gram-CTC decoding ----
  b.call<e2e_gram_ctc_greedy>("e2e_gram_ctc_greedy",
                              "x dtype sB sT sV x_len B T V gram_ids gram_len max_order out out_len cols cols_len stream");
  b.query<e2e_gram_beam_max_width>("e2e_gram_beam_max_width");
  b.query<e2e_gram_beam_workspace_bytes>("e2e_gram_beam_workspace_bytes");
  b.call<e2e_gram_ctc_beam_nbest>("e2e_gram_ctc_beam_nbest",
                                  "lp dtype sB sT sV x_len B T V gram_ids gram_len max_order beam_width nbest out max_out "
                                  "out_len n_hyp scores workspace workspace_bytes stream");
  b.query<e2e_gram_beam_workspace_bytes_lm>("e2e_gram_beam_workspace_bytes_lm");
  b.call<e2e_gram_ctc_beam_nbest_lm>("e2e_gram_ctc_beam_nbest_lm",
                                     "lp dtype sB sT sV x_len B T V gram_ids gram_len max_order num_base_labels beam_width "
                                     "space_id lm lmwt wip oov_penalty nbest out max_out out_len n_hyp scores counts workspace "
                                     "workspace_bytes stream");
  b.call_opts<e2e_gram_ctc_beam_nbest_opt, gram_beam_opts>("e2e_gram_ctc_beam_nbest_opt", "gram_ctc_beam_nbest_opt",
        "lp dtype sB sT sV x_len B T V gram_ids gram_len max_order num_base_labels beam_width space_id lm lmwt wip oov_penalty "
        "nbest out max_out out_len n_hyp scores counts workspace workspace_bytes stream opts", py::none());
  b.query<e2e_gram_beam_stream_row_bytes>("e2e_gram_beam_stream_row_bytes");
  b.query<e2e_gram_beam_stream_workspace_bytes>("e2e_gram_beam_stream_workspace_bytes");
  b.call_opts<e2e_gram_ctc_beam_stream, gram_beam_opts>("e2e_gram_ctc_beam_stream", "gram_ctc_beam_stream",
        "lp dtype sB sT sV chunk_len B T V gram_ids gram_len max_order num_base_labels beam_width scored space_id lm lmwt wip "
        "oov_penalty state row_bytes max_frames nbest out max_out out_len n_hyp scores counts frames_done workspace "
        "workspace_bytes stream opts", py::none());
  // ... with per-frame label pruning (cutoff_top_n, cutoff_prob behind the stream's arguments; nbest_cut has its `scored`).
  // The signatures alone: tests/test_bindings_cpu.py holds this module's functions to the recording of the hand-written layer,
  // so the engine reaches these through end2end_amd._lib, which types them from SIGNATURES like every other symbol
  b.sig<e2e_gram_beam_cut_max_width>("e2e_gram_beam_cut_max_width");
  b.sig<e2e_gram_beam_cut_workspace_bytes>("e2e_gram_beam_cut_workspace_bytes");
  b.sig<e2e_gram_beam_cut_stream_workspace_bytes>("e2e_gram_beam_cut_stream_workspace_bytes");
  b.sig<e2e_gram_beam_cut_stream_row_bytes>("e2e_gram_beam_cut_stream_row_bytes");
  b.sig<e2e_gram_ctc_beam_nbest_cut>("e2e_gram_ctc_beam_nbest_cut");
  b.sig<e2e_gram_ctc_beam_stream_cut>("e2e_gram_ctc_beam_stream_cut");

  // ---- ASG decoding ----
  b.query<e2e_asg_beam_max_width>("e2e_asg_beam_max_width");
  b.query<e2e_asg_beam_workspace_bytes>("e2e_asg_beam_workspace_bytes");
  b.sig<e2e_asg_beam_nbest>("e2e_asg_beam_nbest");
  b.call_opts<e2e_asg_beam_nbest_opt, asg_beam_opts>("e2e_asg_beam_nbest_opt", "asg_beam_nbest",
        "x dtype sB sT sV transitions x_len B T V num_replabels beam_width space_id lm lmwt wip oov_penalty nbest out max_out "
        "out_len n_hyp scores counts workspace workspace_bytes stream restrict_to_lexicon timesteps", false, (uintptr_t)0);
  b.query<e2e_asg_beam_stream_row_bytes>("e2e_asg_beam_stream_row_bytes");
  b.query<e2e_asg_beam_stream_workspace_bytes>("e2e_asg_beam_stream_workspace_bytes");
  b.call_opts<e2e_asg_beam_stream, asg_beam_opts>("e2e_asg_beam_stream", "asg_beam_stream",
        "x dtype sB sT sV transitions chunk_len B T V num_replabels beam_width space_id lm lmwt wip oov_penalty state row_bytes "
        "max_frames nbest out max_out out_len n_hyp scores counts frames_done workspace workspace_bytes stream "
        "restrict_to_lexicon timesteps", false, (uintptr_t)0);
  // ... with per-frame label pruning (cutoff_top_n behind the unpruned calls' arguments).  The signatures alone, as for the
  // pruned Gram-CTC entries above: the engine reaches these through end2end_amd._lib
  b.sig<e2e_asg_beam_cut_workspace_bytes>("e2e_asg_beam_cut_workspace_bytes");
  b.sig<e2e_asg_beam_cut_stream_workspace_bytes>("e2e_asg_beam_cut_stream_workspace_bytes");
  b.sig<e2e_asg_beam_nbest_cut>("e2e_asg_beam_nbest_cut");
  b.sig<e2e_asg_beam_stream_cut>("e2e_asg_beam_stream_cut");

  // ---- CTC decoding ----
  b.call<e2e_ctc_greedy>("e2e_ctc_greedy", "x dtype sB sT sV x_len B T V blank out out_len stream");
  b.query<e2e_ctc_beam_workspace_bytes>("e2e_ctc_beam_workspace_bytes");
  b.query<e2e_ctc_beam_workspace_bytes_lm>("e2e_ctc_beam_workspace_bytes_lm");
  b.query<e2e_ctc_beam_max_width>("e2e_ctc_beam_max_width");
  b.call<e2e_ctc_beam>("e2e_ctc_beam",
                       "lp dtype sB sT sV x_len B T V blank beam_width space_id lm lmwt wip oov_penalty out max_out out_len "
                       "workspace workspace_bytes stream");
  b.query<e2e_ctc_beam_nbest_workspace_bytes>("e2e_ctc_beam_nbest_workspace_bytes");
  b.sig<e2e_ctc_beam_nbest>("e2e_ctc_beam_nbest");
  b.call_opts<e2e_ctc_beam_nbest_opt, ctc_beam_opts>("e2e_ctc_beam_nbest_opt", "ctc_beam_nbest",
        "lp dtype sB sT sV x_len B T V blank beam_width space_id lm lmwt wip oov_penalty nbest out max_out out_len n_hyp scores "
        "counts timesteps workspace workspace_bytes stream restrict_to_lexicon", false);
  b.query<e2e_ctc_beam_stream_row_bytes>("e2e_ctc_beam_stream_row_bytes");
  b.query<e2e_ctc_beam_stream_workspace_bytes>("e2e_ctc_beam_stream_workspace_bytes");
  b.call_opts<e2e_ctc_beam_stream, ctc_beam_opts>("e2e_ctc_beam_stream", "ctc_beam_stream",
        "lp dtype sB sT sV chunk_len B T V blank beam_width space_id lm lmwt wip oov_penalty state row_bytes max_frames "
        "with_timesteps nbest out max_out out_len n_hyp scores counts timesteps frames_done workspace workspace_bytes stream "
        "restrict_to_lexicon", false);

  // per-frame label pruning: the selection alone, and the pruned searches (cutoff_top_n, cutoff_prob behind the unpruned
  // calls' arguments)
  b.query<e2e_ctc_label_cut_max>("e2e_ctc_label_cut_max");
  b.query<e2e_ctc_label_cut_workspace_bytes>("e2e_ctc_label_cut_workspace_bytes");
  b.call<e2e_ctc_label_cut>("e2e_ctc_label_cut",
                            "lp dtype sB sT sV x_len B T V blank cutoff_top_n cutoff_prob ids n workspace workspace_bytes stream");
  b.query<e2e_ctc_beam_cut_max_width>("e2e_ctc_beam_cut_max_width");
  b.query<e2e_ctc_beam_cut_workspace_bytes>("e2e_ctc_beam_cut_workspace_bytes");
  b.query<e2e_ctc_beam_cut_stream_workspace_bytes>("e2e_ctc_beam_cut_stream_workspace_bytes");
  b.call_opts<e2e_ctc_beam_nbest_cut, ctc_beam_opts>("e2e_ctc_beam_nbest_cut", "ctc_beam_nbest_cut",
        "lp dtype sB sT sV x_len B T V blank beam_width space_id lm lmwt wip oov_penalty nbest out max_out out_len n_hyp scores "
        "counts timesteps workspace workspace_bytes stream restrict_to_lexicon cutoff_top_n cutoff_prob");
  b.call_opts<e2e_ctc_beam_stream_cut, ctc_beam_opts>("e2e_ctc_beam_stream_cut", "ctc_beam_stream_cut",
        "lp dtype sB sT sV chunk_len B T V blank beam_width space_id lm lmwt wip oov_penalty state row_bytes max_frames "
        "with_timesteps nbest out max_out out_len n_hyp scores counts timesteps frames_done workspace workspace_bytes stream "
        "restrict_to_lexicon cutoff_top_n cutoff_prob");

  // ---- alignment, word-segmented CTC ----
  b.query<e2e_ctc_align_workspace_bytes>("e2e_ctc_align_workspace_bytes");
  b.call<e2e_ctc_align>("e2e_ctc_align",
                        "lp dtype sB sT sV targets tgt_stride x_len t_len B T V Smax blank is_ctc out pad_value workspace "
                        "workspace_bytes stream");
  b.query<e2e_ctc_wordseg_table_elems>("e2e_ctc_wordseg_table_elems");
  b.query<e2e_ctc_wordseg_workspace_bytes>("e2e_ctc_wordseg_workspace_bytes");
  b.call<e2e_ctc_wordseg_plan>("e2e_ctc_wordseg_plan",
                               "x dtype sB sT sV align targets tgt_stride x_len t_len B T V Smax blank space min_word_length "
                               "table table_elems pool workspace workspace_bytes stream");
  b.call<e2e_ctc_wordseg_gather>("e2e_ctc_wordseg_gather",
                                 "x dtype sB sT sV targets tgt_stride x_len t_len B T V Smax table pool idx n_idx L S xg tg xlg "
                                 "tlg stream");
  b.call<e2e_ctc_wordseg_finish>("e2e_ctc_wordseg_finish",
                                 "x dtype sB sT sV align B T V table g_grads g_losses g_idx n_idx L last losses grads workspace "
                                 "workspace_bytes stream");

  // ---- the language model: the class below forwards to these ----
  b.sig<e2e_lm_load_arpa>("e2e_lm_load_arpa");
  b.sig<e2e_lm_load_words>("e2e_lm_load_words");
  b.sig<e2e_lm_load_transcriptions>("e2e_lm_load_transcriptions");
  b.sig<e2e_lm_free>("e2e_lm_free");
  b.sig<e2e_lm_order>("e2e_lm_order");
  b.sig<e2e_lm_device>("e2e_lm_device");
  b.sig<e2e_lm_word_index>("e2e_lm_word_index");
  b.sig<e2e_lm_score>("e2e_lm_score");
  b.sig<e2e_lm_enable_lexicon>("e2e_lm_enable_lexicon");
  b.sig<e2e_lm_has_lexicon>("e2e_lm_has_lexicon");
  b.sig<e2e_lm_spelling_class>("e2e_lm_spelling_class");
  b.sig<e2e_lm_is_transcribed>("e2e_lm_is_transcribed");
  b.sig<e2e_lm_transcriptions_dropped>("e2e_lm_transcriptions_dropped");
  b.sig<e2e_lm_transcribe>("e2e_lm_transcribe");
  b.sig<e2e_lm_word_string>("e2e_lm_word_string");

  // ---- the diagnostics (include/e2e_ctc_debug.h): reached through end2end_amd._lib only ----
  b.sig<e2e_debug_stream_copy>("e2e_debug_stream_copy");
  b.sig<e2e_debug_occupy>("e2e_debug_occupy");
  b.sig<e2e_debug_loss_route>("e2e_debug_loss_route");
  b.sig<e2e_debug_chain_lean_input>("e2e_debug_chain_lean_input");
  b.sig<e2e_debug_fast_state>("e2e_debug_fast_state");
  b.sig<e2e_debug_fast_redo_failures>("e2e_debug_fast_redo_failures");
  b.sig<e2e_debug_gram_redo_flags>("e2e_debug_gram_redo_flags");
  b.sig<e2e_debug_noblank_redo_flags>("e2e_debug_noblank_redo_flags");
  b.sig<e2e_debug_flagged_phases>("e2e_debug_flagged_phases");
  b.sig<e2e_debug_flagged_counters>("e2e_debug_flagged_counters");
  b.sig<e2e_debug_band_misses>("e2e_debug_band_misses");
  b.sig<e2e_debug_segment_band>("e2e_debug_segment_band");

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
