"""CPU: the C-ABI library loads and exports every symbol include/e2e_ctc.h declares; host logic."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(names=("e2e_ctc.h", "e2e_ctc_debug.h")):
    found = set()
    for name in names:
        hdr = open(os.path.join(ROOT, "include", name)).read()
        hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
        hdr = re.sub(r"#ifdef E2E_[A-Z]+_PROFILE.*?#endif", "", hdr, flags=re.S)     # instrumented builds only
        found |= set(re.findall(r"\b(e2e_[a-z0-9_]+)\s*\(", hdr))
    return found


def _exported():
    from end2end_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("e2e_")}


def test_library_exports_every_declared_symbol():
    from end2end_amd import _lib
    L = _lib.load()
    names = _declared()
    assert {"e2e_ctc_loss_fwd_bwd", "e2e_ctc_greedy", "e2e_ctc_beam", "e2e_lm_load_arpa", "e2e_ctc_align"} <= names
    for n in sorted(names):
        assert hasattr(L, n), n
    assert L.e2e_ctc_abi_version() == _lib.ABI_VERSION


def test_header_declares_every_exported_symbol():
    # the other direction: nothing hides outside the headers -- the contract in e2e_ctc.h, the diagnostics that
    # bench.py and tools/diag use in e2e_ctc_debug.h
    extra = _exported() - _declared()
    assert not extra, "exported but declared in neither include/e2e_ctc.h nor e2e_ctc_debug.h: %s" % sorted(extra)
    assert all(n.startswith("e2e_debug_") for n in _declared(("e2e_ctc_debug.h",)))
    assert not any(n.startswith("e2e_debug_") for n in _declared(("e2e_ctc.h",)))


def test_no_kernel_copies_its_parameter_block_to_scratch():
    """The performance guard that needs no GPU.  A kernel whose parameter struct has its address taken -- handed by reference
    to a function the compiler decides not to inline, which depends on how much code sits around it -- keeps the struct in
    private memory: every wave stores the whole kernarg segment to scratch at its entry (84 dwords per lane for ExactParams,
    before any early exit) and reads its fields back from there.  That is what made the flagged-utterance launch take 9.6 instead
    of 5.3 us, the headline call 132.7 instead of 126.1, in some builds of round 5 (profiles/r05_placement/), with the source of the
    executed path unchanged.  tools/perf/entry_audit.py disassembles the built library's device code and counts the dwords a
    kernel stores to scratch in its first 200 instructions; a handful (a saved register) is normal, a parameter block is not."""
    import shutil
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools", "perf"))
    import entry_audit
    from end2end_amd import _lib
    tools = [os.path.join(entry_audit.LLVM, t) for t in ("llvm-objdump", "llvm-readelf", "clang-offload-bundler")]
    if not all(os.path.exists(t) for t in tools) or not shutil.which("objcopy") or not shutil.which("c++filt"):
        pytest.skip("the ROCm LLVM binutils are not on this machine")
    res = entry_audit.audit(_lib.LIB_PATH)
    assert len(res) >= 60, "the audit found only %d kernels: is the library's device code still bundled the same way?" % len(res)
    assert any("ctc_exact_kernel<float, true, false>" in k for k in res) and any("ctc_fast_segment_kernel<4, false, false>" in k for k in res)
    bad = {k: v for k, v in res.items() if v[0] > 16}
    assert not bad, "kernels that spill a block of state at their entry (dwords stored to scratch, scratch loads): %s" % bad


def test_native_sources_have_no_build_or_environment_switches():
    """One path per shape: no preprocessor switch or environment variable in end2end_amd/csrc selects alternative code.  An A/B
    experiment lives on a branch (tools/diag/build_variant.sh, ab_time.py) and is not merged.  What may stay: include guards,
    the two instrumented builds, and the environment variables the tests use to force a kernel onto a shape the dispatch gives
    to another (E2E_F1_F32 / _SINGLE / _HALO, E2E_BEAM_GENERAL) or to see the n-gram tables' diagnostics (E2E_LM_DEBUG)."""
    profile_builds = {"E2E_FAST_PROFILE", "E2E_BEAM_PROFILE"}
    kept_env = {"E2E_F1_F32", "E2E_F1_SINGLE", "E2E_F1_HALO", "E2E_BEAM_GENERAL", "E2E_LM_DEBUG"}
    csrc = os.path.join(ROOT, "end2end_amd", "csrc")
    conds, envs, sources = [], set(), 0
    for dirpath, _, files in os.walk(csrc):
        for f in sorted(files):
            if not f.endswith((".hip", ".h", ".hpp", ".cpp", ".cc", ".c")):
                continue
            sources += 1
            rel = os.path.relpath(os.path.join(dirpath, f), ROOT)
            text = open(os.path.join(dirpath, f)).read()
            lines = text.splitlines()
            for i, line in enumerate(lines):
                m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif|elifdef|elifndef)\b(.*)", line)
                if not m:
                    continue
                cond = re.sub(r"/\*.*?\*/", "", m.group(2).split("//")[0]).strip()
                name = re.sub(r"^defined\s*\(?\s*(\w+)\s*\)?$", r"\1", cond) if m.group(1) == "if" else cond
                guard = (m.group(1) == "ifndef" and i + 1 < len(lines)
                         and re.fullmatch(r"\s*#\s*define\s+%s\s*" % re.escape(cond), lines[i + 1]) is not None)
                if not guard and name not in profile_builds:
                    conds.append("%s:%d: %s" % (rel, i + 1, line.strip()))
            code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
            for m in re.finditer(r"getenv\s*\(\s*([^)]*)\)", code):
                lit = re.fullmatch(r'"([^"]*)"', m.group(1).strip())
                envs.add(lit.group(1) if lit else "<not a literal: %s in %s>" % (m.group(1).strip(), rel))
    assert sources >= 8, "found only %d native sources under %s" % (sources, csrc)
    assert not conds, "preprocessor conditions other than include guards and %s:\n%s" % (sorted(profile_builds), "\n".join(conds))
    assert envs <= kept_env, "environment variables read beyond %s: %s" % (sorted(kept_env), sorted(envs - kept_env))


def test_pybind_layer_loads_and_reports_errors():
    from end2end_amd import _C, _runtime
    assert _C.abi_version() == _C.ABI_VERSION == _runtime.ABI_VERSION
    assert _C.ctc_loss_workspace_bytes(4, 50, 28, 30, _C.F32, _C.ALGO_AUTO) > 0
    with pytest.raises(_C.E2EError, match="dtype"):          # argument checks run before any GPU call
        _C.ctc_loss_fwd_bwd(0, 5, True, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0)
    assert issubclass(_C.E2EError, RuntimeError)


def test_reference_module_names_resolve_to_the_engines():
    # pytorch_end2end/modules/ctc_loss.py:74 (import_module("cpp_ctc_loss")), decoders/ctc_decoder.py:13
    import inspect
    from importlib import import_module
    loss_mod, dec_mod = import_module("cpp_ctc_loss"), import_module("cpp_ctc_decoder")
    eng = loss_mod.CTCLossEngine(0)
    assert list(inspect.signature(eng.compute).parameters)[:4] == ["logits", "targets", "logits_lengths", "targets_lengths"]
    sig = inspect.signature(dec_mod.CTCDecoder.__init__)
    got = [(k, v.default) for k, v in sig.parameters.items() if k not in ("self", "keep_on_device")]
    assert got[0][0] == "blank_idx"
    # keyword names and defaults of src/decoders/ctc_decoder_py.cpp:17-24
    assert [(k, (d or type(d)())) for k, d in got[1:]] == [("beam_width_", 100), ("labels", type(None)()), ("lm_path", ""),
                                                         ("lmwt_", 1.0), ("wip_", 0.0), ("oov_penalty_", -1000.0),
                                                         ("case_sensitive", False)]
    for name in ("decode", "decode_greedy"):
        assert list(inspect.signature(getattr(dec_mod.CTCDecoder, name)).parameters)[1:] == ["logits_", "logits_lengths_"]
    assert list(inspect.signature(dec_mod.CTCDecoder.print_scores_for_sentence).parameters)[1:] == ["words"]
    import pytorch_end2end
    import end2end_amd
    assert pytorch_end2end.CTCLoss is end2end_amd.CTCLoss and pytorch_end2end.CTCDecoder is end2end_amd.CTCDecoder
    assert pytorch_end2end.CTCEncoder is end2end_amd.CTCEncoder
    from pytorch_end2end.modules.ctc_loss import CTCLoss as A
    from pytorch_end2end.decoders.ctc_decoder import CTCDecoder as B, CTCDecoderError  # noqa: F401
    from pytorch_end2end.functions.forward_backward import ForwardBackwardLossFunction  # noqa: F401
    assert A is end2end_amd.CTCLoss and B is end2end_amd.CTCDecoder


def test_no_cpu_fallback_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from end2end_amd import CTCLoss, CTCDecoder
    x = torch.randn(2, 5, 4, requires_grad=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CTCLoss()(x, torch.tensor([[1, 2], [1, 2]]), torch.tensor([5, 5]), torch.tensor([2, 2]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CTCDecoder(beam_width=1).decode(x)


def test_product_does_not_import_the_oracle():
    import end2end_amd
    pkg = os.path.dirname(end2end_amd.__file__)
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(d, f)).read()
                assert "oracle_lib" not in src and "liboracle" not in src and "oracle/" not in src.replace("oracle/.", ""), f


def test_encoder_matches_captured_reference_io():
    from end2end_amd import CTCEncoder
    for c in G.encoder_cases():
        tf = str.upper if c["transform"] == "upper" else str.lower
        e = CTCEncoder(c["characters"], c["blank_id"], tf)
        assert e.clean(c["text"]) == c["clean"]
        assert e.encode(c["text"]).tolist() == c["encode"]
        assert e.num_symbols == c["num_symbols"]
        assert e.decode(c["decode_in"]) == c["decode_out"]
        assert e.decode_pure(c["decode_in"]) == c["decode_pure_out"]


def test_decoder_wrapper_parameter_checks(tmp_path):
    from end2end_amd import CTCDecoder, CTCDecoderError
    with pytest.raises(CTCDecoderError, match="Can't find a model"):
        CTCDecoder(labels=["_", "a"], lm_path=str(tmp_path / "missing.arpa"))
    with pytest.raises(CTCDecoderError, match="Can't find a model"):     # the labels check upstream can never fire
        CTCDecoder(lm_path=str(tmp_path / "missing.arpa"))
    d = CTCDecoder(beam_width=1, labels=["_", "a", " "])
    assert d._decoder.space_id == 2 and d._decoder.lmwt == 0.0
    assert d._wip == 1.0 and d._oov_penalty == -10 and d._case_sensitive is True   # wrapper defaults
    from end2end_amd.engines import CTCDecoderEngine
    e = CTCDecoderEngine(0)
    assert (e.beam_width, e.wip, e.oov_penalty, e.case_sensitive) == (100, 0.0, -1000.0, False)  # engine defaults


def test_beam_width_limits_are_queryable_and_enforced_at_construction():
    from end2end_amd import _C
    from end2end_amd.engines import CTCDecoderEngine
    # the fast kernel's range is bounded by the alphabet; beyond it the general kernel takes over, up to width 512
    for V in (4, 29, 200, 8000):
        assert _C.ctc_beam_max_width(V, False) == 512 and _C.ctc_beam_max_width(V, True) == 512
    labels = ["_"] + ["l%d" % i for i in range(199)]
    CTCDecoderEngine(0, 512, labels)
    with pytest.raises(ValueError, match="beam_width"):
        CTCDecoderEngine(0, 513, labels)
    CTCDecoderEngine(0, 1, labels)           # greedy has no such limit
    assert _C.ctc_beam_workspace_bytes(8, 256, 8000, 100) > 8 * 100 * 8000 * 8
    # a call without a language model does not pay for the LM's answer rows, the one-workgroup kernel for nothing of the general one
    no_lm, with_lm = _C.ctc_beam_workspace_bytes_lm(8, 256, 8000, 100, False), _C.ctc_beam_workspace_bytes_lm(8, 256, 8000, 100, True)
    assert 8 * 100 * 8000 * 8 < no_lm < 0.45 * with_lm and with_lm == _C.ctc_beam_workspace_bytes(8, 256, 8000, 100)
    assert _C.ctc_beam_workspace_bytes_lm(64, 1500, 29, 100, False) < 64 * 100 * 1503 * 8 + (1 << 20)


def test_kenlm_binary_models_are_refused_with_a_clear_message(tmp_path):
    from end2end_amd.engines import LanguageModel
    from end2end_amd._runtime import E2EError
    p = tmp_path / "model.binary"
    p.write_bytes(b"mmap lm http://kheafield.com/code format version 5\n\x00" + bytes(200))
    with pytest.raises(E2EError, match="KenLM binary"):
        LanguageModel(str(p), ["_", "a"], True)


def test_bench_helpers(tmp_path, monkeypatch):
    """bench.py's host-side pieces: the recorded PMC traffic is found for the headline workload, the synthetic ARPA is
    deterministic, the options parse (a plain run is lean, a step count must be positive), and `--gpus N` without a
    launcher starts N ranks through torch.distributed.run on 127.0.0.1."""
    import bench
    a = bench.parse_args([])
    assert not a.full and a.dump_outputs is None
    a = bench.parse_args(["--steps", "3", "--warmup", "0", "--full", "--dump-outputs", "d"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (3, 0, True, "d")
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)
    t = bench.recorded_traffic(bench.WORKLOAD["name"])
    assert t is not None and 1.5e8 < t < 3.5e8
    labels = ["_"] + [chr(97 + i) for i in range(26)] + [" ", "'"]
    a, b = tmp_path / "a.arpa", tmp_path / "b.arpa"
    bench.synthetic_arpa(str(a), labels, n_words=200, seed=3)
    bench.synthetic_arpa(str(b), labels, n_words=200, seed=3)
    assert a.read_text() == b.read_text() and "\\3-grams:" in a.read_text()
    seen = {}
    monkeypatch.setattr(bench.subprocess, "call", lambda cmd, env=None: seen.update(cmd=cmd, env=env) or 0)
    monkeypatch.setattr(bench.sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])

    class A:
        gpus = 4
    assert bench.launch_ranks(A) == 0
    cmd = seen["cmd"]
    assert "torch.distributed.run" in cmd and "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-4:] == ["--gpus", "4", "--steps", "3"]
    assert seen["env"].get("HSA_ENABLE_IPC_MODE_LEGACY") == "0"


def test_workspace_of_the_headline_shape_stays_under_250_megabytes():
    # 924 MB (256 alpha slabs of the flagged-utterance launch) -> the fast path's own 100 MB + 24 slabs;
    # round 5: + 66 MB, one int exponent per checkpoint cell for the extended-range redo (ctc_ext.h)
    from end2end_amd import _lib
    L = _lib.load()
    n = L.e2e_ctc_loss_workspace_bytes(256, 1000, 29, 200, _lib.F32, _lib.ALGO_AUTO)
    assert 50e6 < n <= 250e6, n
    # and it no longer grows with the batch beyond the fast path's own share
    n4 = L.e2e_ctc_loss_workspace_bytes(1024, 1000, 29, 200, _lib.F32, _lib.ALGO_AUTO)
    assert n4 - n < 3.2 * (n - 77e6), (n, n4)


def test_language_model_kernel_tables_pass_their_self_check(tmp_path):
    """The loader builds what the beam kernel reads -- a two-choice vocabulary table carrying each word's unigram, a
    direct-indexed unigram array, hashed n-gram signatures with continuation bits -- and checks all of it against the id
    tables (every spelling found with its id, every listed n-gram found with its numbers, every context listing its
    continuations) before using it; a failed check (or a failed cuckoo insertion) falls back to the id tables.  Runs on the
    host: no GPU needed."""
    import bench
    labels = ["_"] + [chr(97 + i) for i in range(26)] + [" ", "'"]
    big = str(tmp_path / "synthetic.arpa")
    bench.synthetic_arpa(big, labels, n_words=20000, seed=5)
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from end2end_amd.engines import LanguageModel\n"
            "for path, cs in ((%r, False), (%r, True), (%r, False)):\n"
            "    lm = LanguageModel(path, %r, cs)\n"
            "    assert lm.order() == 3\n") % (ROOT, big, big, os.path.join(ROOT, "tests", "golden", "tiny_3gram.arpa"), labels)
    r = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, env={**os.environ, "E2E_LM_DEBUG": "1"})
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stderr.splitlines() if l.startswith("e2e_lm:")]
    assert len(lines) == 3 and all(l.endswith("signature tables ok") for l in lines), r.stderr


def test_language_model_with_an_unlisted_context_uses_the_id_tables(tmp_path):
    """SRILM-pruned ARPA files can list an n-gram whose context is missing (KenLM inserts blank entries for those).  The beam
    kernel's signature tables look an n-gram up only behind a hit of its context, so such a model must fall back to the
    id-keyed walk, and the host scorer must still find the n-gram (here: trigram 'a b a' without bigram 'a b')."""
    src = open(os.path.join(ROOT, "tests", "golden", "tiny_3gram.arpa")).read()
    pruned = src.replace("-0.6\ta b\t-0.2\n", "").replace("ngram 2=5", "ngram 2=4")
    assert pruned != src
    path = str(tmp_path / "pruned.arpa")
    open(path, "w").write(pruned)
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from end2end_amd.engines import LanguageModel\n"
            "lm = LanguageModel(%r, ['_', 'a', 'b', ' '], True)\n"
            "a, b = lm.word_index('a'), lm.word_index('b')\n"
            "print('SCORE %%.6f' %% lm.score([b, a], a))\n") % (ROOT, path)
    r = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, env={**os.environ, "E2E_LM_DEBUG": "1"})
    assert r.returncode == 0, r.stderr
    assert "SCORE -0.250000" in r.stdout, r.stdout              # the trigram itself, not the backed-off -0.5
    lines = [l for l in r.stderr.splitlines() if l.startswith("e2e_lm:")]
    assert any("context is not listed" in l for l in lines) and any(l.endswith("signature tables NOT usable") for l in lines), r.stderr


def test_one_character_labels_that_are_lone_surrogates_still_spell():
    """indices2str for the whole batch goes through a UTF-32 table; a lone surrogate (a legal one-character Python label) is not
    valid UTF-32, so such alphabets keep the per-id join instead of raising UnicodeDecodeError."""
    import torch
    from end2end_amd.engines import CTCDecoderEngine as DecoderEngine
    eng = DecoderEngine(0, 1, ["_", "\ud800", "a"])
    assert eng._codes is None
    assert eng._strings(torch.tensor([[1, 2, 0], [2, 2, 2]]), [2, 3]) == ["\ud800a", "aaa"]
    plain = DecoderEngine(0, 1, ["_", "b", "a"])
    assert plain._codes is not None and plain._strings(torch.tensor([[1, 2, 0], [2, 2, 2]]), [2, 3]) == ["ba", "aaa"]


def test_loss_route_at_the_band_edges():
    """e2e_debug_loss_route -- computed by the functions the loss call dispatches with (resolve_algo, use_wide, wide_row_form,
    ppl_of, chain_rule), on the host -- at the edges README / DESIGN name.  It is the WIDTH of the targets tensor that moves a
    call from band to band: tests/test_gpu_fuzz.py's callshape family pads its way through all of them."""
    import gpu_util as U
    from end2end_amd import _lib
    f32, f64, bf16 = _lib.F32, _lib.F64, _lib.BF16
    AUTO, EXACT, FAST = _lib.ALGO_AUTO, _lib.ALGO_EXACT, _lib.ALGO_FAST

    def route(B, T, V, S, dtype=f32, algo=AUTO, **kw):
        return U.loss_route(dtype, algo, B, T, V, S, **kw)

    # widths 63/64, 127/128, 223/224, 255/256, 447/448 at 29 columns: pairs per lane 1, 2, 4, 4, 8; the lean halo chains (rule 4)
    # up to 223 labels, the single-wave chains (6) for one pair per lane and for 224..255 labels, ChainF64L (2) for eight pairs
    got = [route(8, 1000, 29, S) for S in (1, 63, 64, 127, 128, 223, 224, 255, 256, 447, 448, 600)]
    assert got == [2016, 2016, 2024, 2024, 2044, 2044, 2046, 2046, 2082, 2082, 1000, 1000], got
    assert route(8, 1000, 29, 200, chains=_lib.CHAINS_F32) == 2043 and route(8, 1000, 29, 100, chains=_lib.CHAINS_F32) == 2024
    # B 256/257 at two pairs per lane: beyond one utterance per CU the single-wave chains; their ring of four blocks (7)
    # where eight need more than 80 KB of LDS (63..96 columns).  The lean halo chains hold up to 78 columns: beyond, ChainF64 (5)
    # at four pairs per lane and the single-wave chains at two
    assert [route(B, 1000, 29, 100) for B in (256, 257)] == [2024, 2026]
    assert [route(B, 256, V, 64) for B, V in ((512, 62), (512, 63), (512, 96), (256, 78), (256, 79))] == [2026, 2027, 2027, 2024, 2026]
    assert [route(8, 1000, V, 200) for V in (78, 79, 96)] == [2044, 2045, 2045]
    # 96/97, 224/225, 448/449 columns: the wide-row forms (rule 1) with four, then eight pairs per lane, then the compaction
    got = [route(8, 1000, V, 100) for V in (96, 97, 224, 225, 448, 449, 452)]
    assert got == [2026, 2041, 2041, 2081, 2081, 3041, 3241], got
    # eight pairs per lane: ChainF64L's ring fits the LDS up to 73 columns, the wide-row form beyond
    assert [route(8, 1000, V, 300) for V in (29, 73, 74, 96, 150, 224)] == [2082, 2082, 2081, 2081, 2081, 2081]
    assert route(8, 1000, 150, 223) == 2041 and route(8, 1000, 150, 224) == 2081
    # the compaction: its lattice has Smax + 1 columns, so the WIDTH picks the inner kernels as well; the row kernels follow
    # the alphabet, the strides and the alignment
    got = [route(8, 1000, 8000, S) for S in (63, 64, 77, 78, 95, 96, 223, 224, 447, 448)]
    assert got == [3416, 3424, 3424, 3426, 3426, 3441, 3441, 3481, 3481, 4400], got
    assert [route(8, 1000, V, 50) for V in (1000, 1001, 2048, 2052, 4096, 4100, 8192, 8196)] == [3216, 3016, 3216, 3316, 3316, 3416, 3416, 3116]
    assert route(8, 1000, 8000, 50, sV=2) == 3016 and route(8, 1000, 8000, 50, x=260) == 3016
    assert route(8, 1000, 8000, 50, dtype=bf16) == 3416 and route(8, 1000, 8004, 50, dtype=bf16) == 3016
    assert route(8, 1000, 1000, 600) == 1000 and route(8, 1000, 1204, 600) == 4200        # (the compaction must halve the columns)
    # what is refused, and what is the exact kernel's
    assert route(8, 1000, 29, 100, dtype=f64) == 1000 and route(8, 1000, 29, 100, algo=EXACT) == 1000
    assert route(8, 1000, 29, 448, algo=FAST) == -1 and route(8, 1000, 8000, 448, algo=FAST) == -1
    assert route(8, 1000, 29, 448, dtype=bf16) == -1 and route(8, 1000, 29, 100, dtype=bf16, algo=EXACT) == -1
    assert route(8, 1000, 29, 100, algo=FAST) == 2024 and route(8, 0, 29, 100) == -1
    # the workspace steps where the route does (its layout follows the same ppl_of: 128 checkpoint cells per pair per lane)
    L = _lib.load()
    ws = lambda S: L.e2e_ctc_loss_workspace_bytes(8, 1000, 29, S, f32, AUTO)
    for S in (63, 127, 255):
        assert ws(S + 1) - ws(S) > 8 * (ws(S) - ws(S - 1)) > 0, S
