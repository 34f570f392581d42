"""CPU checks of the n-gram language model (csrc/ngram_lm.cpp behind pk_lm_load_buffer / pk_lm_score): scores
against the dictionary scorer of tests/ngram_lm_ref.py BIT FOR BIT, every refusal of the loader with its line, hostile buffers, and the new
C ABI symbols (declared, exported, bound; the fused entry points refuse bad arguments before they look for a device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from parakeet_cpp_amd import capi

import ngram_lm_ref as NR

HEADER = os.path.join(ROOT, "include", "parakeet_amd.h")
LM_SYMBOLS = ["pk_lm_load", "pk_lm_load_buffer", "pk_lm_free", "pk_lm_order", "pk_lm_num_ngrams", "pk_lm_score", "pk_lm_options_default",
              "pk_ctc_beam_search_lm", "pk_ctc_beam_decode_lm", "pk_ctc_beam_decode_lm_ragged", "pk_ctc_beam_decode_lm_timed",
              "pk_transcribe_pcm_nbest_lm"]


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def strings_for(V, rng, n=60, extra=()):
    out = [[]]
    for _ in range(n):
        L = int(rng.integers(1, 14))
        pool = 4 if rng.random() < 0.6 else V - 1                   # short alphabets meet the higher orders, the whole alphabet backs off
        out.append([int(x) for x in rng.integers(0, pool, size=L)])
    return out + [list(e) for e in extra]


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("density", [0.5, 3.0])
@pytest.mark.parametrize("unk,bos", [(False, False), (True, False), (False, True), (True, True)])
def test_score_equals_the_dictionary_scorer_bit_for_bit(order, density, unk, bos):
    V = 9
    text = NR.make_arpa(V, order, density, unk, bos, seed=order * 10 + int(density) + 2 * unk + bos)
    ref, lm = NR.RefLm(text), capi.Lm.from_text(text)
    assert lm.order == order and lm.num_ngrams == len(ref.table)
    rng = np.random.default_rng(order)
    extra = ([[V + 3], [0, V + 3, 1], [300000, 2]] if unk else [])  # ids the file never names: <unk>
    strs = strings_for(V, rng, extra=extra)
    if unk:
        assert any(ref.table.get((c,)) is None for s in strs for c in s), "degenerate: no <unk> hit"
    for use_bos in (True, False):
        for use_eos in ((False, True) if (bos or unk) else (False,)):   # </s> needs an entry or <unk>
            got = lm.score(strs, bos=use_bos, eos=use_eos)
            want = np.array([ref.score(s, use_bos, use_eos) for s in strs], np.float32)
            assert np.array_equal(bits(got), bits(want)), (use_bos, use_eos)
    assert bits(lm.score([[]], bos=True, eos=False))[0] == 0        # the empty string: +0.0
    lm.close()


def test_back_off_chains_of_every_length_are_scored():
    """order 5, sparse: lookups that add 0, 1, 2, 3 and 4 back-off weights all occur among the scored strings (asked of the reference)."""
    V, order = 9, 5
    text = NR.make_arpa(V, order, 0.9, False, True, seed=77)
    ref, lm = NR.RefLm(text), capi.Lm.from_text(text)
    rng = np.random.default_rng(3)
    strs = strings_for(V, rng, n=400)
    strs += [list(g) for g in ref.table if len(g) == 5 and all(isinstance(w, int) for w in g)]      # the 5-grams themselves: chains of length 0
    seen = set()
    for s in strs:
        hist = ref.start(True)
        for c in s:
            seen.add((len(tuple(hist[-(order - 1):])), ref.lookup(hist, c)[2]))
            hist = hist + (c,)
    assert np.array_equal(bits(lm.score(strs)), bits([ref.score(s) for s in strs]))
    lm.close()
    # the full chain needs a 4-word context whose every suffix is an entry: written by hand
    grams = [[(i,) for i in range(8)], [(1, 2), (2, 3), (3, 4)], [(1, 2, 3), (2, 3, 4)], [(1, 2, 3, 4)], [(1, 2, 3, 4, 6)]]
    lines = ["\\data\\"] + [f"ngram {k + 1}={len(g)}" for k, g in enumerate(grams)]
    for k, gs in enumerate(grams):
        lines += ["", f"\\{k + 1}-grams:"] + [f"-{0.3 + 0.11 * j + 0.07 * k:.4f}\t{' '.join(map(str, g))}" + (f"\t-{0.2 + 0.013 * j + 0.1 * k:.4f}" if k < 4 else "")
                                              for j, g in enumerate(gs)]
    text = "\n".join(lines + ["", "\\end\\", ""])
    ref, lm = NR.RefLm(text), capi.Lm.from_text(text)
    strs = [[1, 2, 3, 4, 5], [1, 2, 3, 4, 6], [0, 1, 2, 3, 4, 5, 1, 2, 3, 4, 6], [2, 3, 4, 7], [3, 4, 4]]
    for s in strs:
        hist = ref.start(True)
        for c in s:
            seen.add((len(tuple(hist[-(order - 1):])), ref.lookup(hist, c)[2]))
            hist = hist + (c,)
    assert {lv for _, lv in seen} == set(range(order)), sorted(seen)
    assert np.array_equal(bits(lm.score(strs)), bits([ref.score(s) for s in strs]))
    lm.close()


def test_values_are_converted_once_through_double():
    text = "\\data\\\nngram 1=2\nngram 2=1\n\n\\1-grams:\n-0.1\t0\t-0.7\n-1.23456789012\t1\n\n\\2-grams:\n-2.5e-1\t0 1\n\n\\end\\\n"
    lm = capi.Lm.from_text(text)
    f = lambda s: np.float32(float(s) * 2.302585092994046)
    assert bits(lm.score([[0]]))[0] == bits(f("-0.1")) and bits(lm.score([[1]]))[0] == bits(f("-1.23456789012"))
    assert bits(lm.score([[0, 1]]))[0] == bits(np.float32(f("-0.1") + f("-2.5e-1")))
    assert bits(lm.score([[0, 0]]))[0] == bits(np.float32(f("-0.1") + np.float32(np.float32(np.float32(0.0) + f("-0.7")) + f("-0.1"))))
    lm.close()


BASE = ["\\data\\", "ngram 1=4", "ngram 2=2", "", "\\1-grams:", "-1.0\t0\t-0.5", "-1.0\t1\t-0.5", "-2.0\t<unk>", "-1.5\t</s>", "",
        "\\2-grams:", "-0.5\t0 1", "-0.7\t1 </s>", "", "\\end\\"]


def edited(repl=None, insert=None, drop=None):
    lines = list(BASE)
    if repl:
        lines[repl[0] - 1] = repl[1]
    if insert:
        lines.insert(insert[0] - 1, insert[1])
    if drop:
        del lines[drop - 1]
    return "\n".join(lines) + "\n"


REFUSALS = [
    ("a word that is no id", edited(repl=(6, "-1.0\tabc\t-0.5")), 6),
    ("a signed id", edited(repl=(6, "-1.0\t-3\t-0.5")), 6),
    ("an id of 2^24", edited(repl=(6, "-1.0\t16777216\t-0.5")), 6),
    ("more unigrams declared than present", edited(repl=(2, "ngram 1=5")), 11),
    ("fewer bigrams declared than present", edited(repl=(3, "ngram 2=1")), 15),
    ("an order past 5", "\\data\\\n" + "".join(f"ngram {k}=0\n" for k in range(1, 7)), 7),
    ("orders out of sequence", edited(repl=(3, "ngram 3=2")), 3),
    ("a section that was not declared", edited(insert=(15, "\\3-grams:")), 15),
    ("a missing section", edited(repl=(11, "")), 12),
    ("a prefix that is no entry", edited(repl=(12, "-0.5\t7 1")), 12),
    ("a duplicate n-gram", edited(repl=(13, "-0.7\t0 1")), 13),
    ("a duplicate unigram", edited(repl=(7, "-1.0\t0")), 7),
    ("nan", edited(repl=(6, "nan\t0\t-0.5")), 6),
    ("inf as back-off", edited(repl=(6, "-1.0\t0\tinf")), 6),
    ("a value past fp32", edited(repl=(6, "-1e39\t0\t-0.5")), 6),
    ("a value past double", edited(repl=(6, "-1e999\t0\t-0.5")), 6),
    ("a number with a tail", edited(repl=(6, "-1.0x\t0\t-0.5")), 6),
    ("too many columns", edited(repl=(12, "-0.5\t0 1\t-0.1\t-0.2")), 12),
    ("too few columns", edited(repl=(12, "-0.5\t0")), 12),
    ("no <unk> and an id without a unigram", edited(repl=(8, "-2.0\t3"), insert=None).replace("-0.5\t0 1", "-0.5\t0 7"), 12),
    ("no \\end\\", edited(drop=15), 14),
    ("no \\data\\", "hello\nworld\n", 2),
    ("a count that is no number", edited(repl=(2, "ngram 1=four")), 2),
]


@pytest.mark.parametrize("what,text,line", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_loader_refuses_and_names_the_line(what, text, line):
    with pytest.raises(capi.PkError) as e:
        capi.Lm.from_text(text)
    assert e.value.code == -1, what
    assert re.search(rf"line {line}\b", str(e.value)), f"{what}: '{e.value}' does not name line {line}"


def test_the_base_text_of_the_refusals_loads():
    lm = capi.Lm.from_text(edited())
    assert (lm.order, lm.num_ngrams) == (2, 6)
    lm.close()


def test_truncated_and_garbage_buffers_are_refused_never_crash():
    text = NR.make_arpa(9, 3, 1.0, True, True, seed=5).encode()
    end = text.rindex(b"\\end\\") + 5
    for cut in list(range(0, 200)) + list(range(200, end, 37)) + [end - 1]:
        with pytest.raises(capi.PkError) as e:
            capi.Lm.from_text(text[:cut])
        assert e.value.code == -1
    capi.Lm.from_text(text[:end]).close()                           # complete up to \end\ (no newline after it): loads
    rng = np.random.default_rng(9)
    for n in (0, 1, 7, 64, 4096):
        for _ in range(8):
            with pytest.raises(capi.PkError):
                capi.Lm.from_text(bytes(rng.integers(0, 256, size=n, dtype=np.uint8)))
    hostile = [b"\\data\\\nngram 1=99999999999999\n\n\\1-grams:\n-1.0\t0\n\\end\\\n",            # a count nothing is sized by
               b"\\data\\\nngram 1=1\n\\1-grams:\n-1.0\t" + b"9" * 5000 + b"\n\\end\\\n",          # a very long id
               b"\\data\\\nngram 1=1\n\\1-grams:\n" + b"-" * 5000 + b"\t0\n\\end\\\n",             # a very long number
               b"\\data\\\nngram 1=1\n\\1-grams:\n-1.0\t0\x00\n\\end\\\n",                         # a NUL inside a word
               b"\\data\\\n" * 3, b"\\end\\\n", b"\\data\\\n\\end\\\n", b"\\data\\\nngram 1=0\n\\1-grams:\n\\end\\"]
    for h in hostile[:-1]:
        with pytest.raises(capi.PkError) as e:
            capi.Lm.from_text(h)
        assert e.value.code == -1, h[:40]
    lm = capi.Lm.from_text(hostile[-1])                             # an empty model is a model: it scores nothing
    with pytest.raises(capi.PkError):
        lm.score([[0]])
    lm.close()
    mixed = bytearray(text)
    for _ in range(200):                                            # single-byte damage anywhere: an error or a model, never a crash
        m = bytearray(mixed)
        m[int(rng.integers(len(m)))] = int(rng.integers(256))
        try:
            capi.Lm.from_text(bytes(m)).close()
        except capi.PkError as e:
            assert e.code == -1


def test_load_from_a_file_and_io_error(tmp_path):
    text = NR.make_arpa(9, 3, 1.0, True, True, seed=6)
    p = tmp_path / "m.arpa"
    p.write_text(text.replace("\n", "\r\n"))                        # CRLF line ends are fine
    a, b = capi.Lm.load(p), capi.Lm.from_text(text)
    strs = strings_for(9, np.random.default_rng(1))
    assert np.array_equal(bits(a.score(strs, eos=True)), bits(b.score(strs, eos=True)))
    a.close(); b.close()
    with pytest.raises(capi.PkError) as e:
        capi.Lm.load(tmp_path / "missing.arpa")
    assert e.value.code == -2 and "missing.arpa" in str(e.value)


def test_score_refuses_bad_ids():
    lm = capi.Lm.from_text(NR.make_arpa(9, 2, 1.0, False, False, seed=1))
    for bad in ([[-1]], [[0, 1 << 24]], [[8]], [[100]]):             # negative, past 2^24, and (no <unk>) ids without a unigram
        with pytest.raises(capi.PkError) as e:
            lm.score(bad)
        assert e.value.code == -1, bad
    with pytest.raises(capi.PkError):
        lm.score([[0]], eos=True)                                   # no </s>, no <unk>
    lm.close()


def test_lm_symbols_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", txt))
    L = capi.lib()
    for s in LM_SYMBOLS:
        assert s in declared, f"{s} is not declared in include/parakeet_amd.h"
        assert hasattr(L, s), f"{s} is not exported by libparakeet_amd.so"
        assert s in capi._LATE_SIGNATURES, f"{s} has no ctypes signature in capi.py"
    assert "pk_lm_options" in txt and "typedef struct pk_lm pk_lm" in txt
    o = capi.lm_options()
    assert (o.alpha, o.beta) == (0.5, 0.0) and C.sizeof(capi.PkLmOptions) == 8
    assert L.pk_lm_order(None) == 0
    L.pk_lm_free(None)


def test_fused_search_refuses_bad_arguments_before_it_looks_for_a_device():
    V, blank = 9, 8
    lp = np.zeros((1, 3, V), np.float32)
    good = capi.Lm.from_text(NR.make_arpa(V, 2, 1.0, False, False, seed=2))
    names_blank = capi.Lm.from_text(NR.make_arpa(V + 1, 2, 1.0, False, False, seed=2))      # its ids reach V - 1 = the blank
    too_wide = capi.Lm.from_text(NR.make_arpa(V + 2, 2, 1.0, False, False, seed=2))         # an id >= V
    no_cover = capi.Lm.from_text(NR.make_arpa(V - 1, 2, 1.0, False, False, seed=2))         # no <unk>, id V - 2 has no unigram
    for lm, kw in ((names_blank, {}), (too_wide, {}), (no_cover, {}), (good, dict(lm_alpha=float("nan"))), (good, dict(lm_beta=float("inf"))),
                   (good, dict(beam_width=0)), (good, dict(beam_width=4, n_best=5))):
        with pytest.raises(capi.PkError) as e:
            capi.ctc_beam_search(lp, blank, lm=lm, **kw)
        assert e.value.code == -1 and str(e.value), kw
    ids = np.zeros((1, 1, 3), np.int32); lens = np.zeros((1, 1), np.int32)
    st = capi.lib().pk_ctc_beam_search_lm(capi._f(lp), None, 1, 3, V, blank, None, capi._i(ids), capi._i(lens), None, None, None, None, None, None, None)
    assert st == -1                                                 # no model given
    for lm in (good, names_blank, too_wide, no_cover):
        lm.close()


def test_make_token_corpus_writes_the_tokenizers_ids(tmp_path):
    """tools/make_token_corpus.py: one id line per text line, the ids Model.tokenize gives (host only)."""
    import importlib.util
    import io
    from conftest import pk
    from parakeet_cpp_amd import synth
    spec = importlib.util.spec_from_file_location("make_token_corpus", os.path.join(ROOT, "tools", "make_token_corpus.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    cfg = pk.make_tiny_config()
    wp, vp = str(tmp_path / "w.safetensors"), str(tmp_path / "v.txt")
    synth.save_weights(wp, synth.synth_weights(cfg, seed=1))
    vocab = synth.synth_vocab(cfg.vocab_size - 1)
    synth.save_vocab(vp, vocab)
    m = capi.Model(wp, cfg, vocab_path=vp)
    words = [v.replace("▁", " ").strip() for v in vocab if v.startswith("▁")][:3]
    lines = [" ".join(words) + "\n", "\n", words[0].upper() + "\n"]
    out = io.StringIO()
    n_lines, n_tok = tool.convert(m, lines, out, lower=True)
    got = out.getvalue().split("\n")[:-1]
    assert n_lines == 3 and got[1] == "" and len(got) == 3
    assert [int(x) for x in got[0].split()] == m.tokenize(" ".join(words)) and n_tok == len(got[0].split()) + len(got[2].split())
    assert got[2].split() == [str(i) for i in m.tokenize(words[0])] and got[2]
    out = io.StringIO()
    assert tool.convert(m, lines, out, lower=True, skip_empty=True)[0] == 2
    m.close()
