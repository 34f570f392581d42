#!/usr/bin/env python3
"""Text lines -> token-id lines through the model's own tokenizer (Model.tokenize / pk_tokenize): the corpus an n-gram trainer (KenLM's lmplz,
SRILM's ngram-count, ...) turns into an ARPA file whose words are decimal token ids -- the only kind pk_lm_load reads (DESIGN.md section
5.5.6).  One output line per input line: the ids separated by blanks; empty lines stay empty unless --skip-empty.  Needs no GPU: the model
is loaded on the host only.
usage: python tools/make_token_corpus.py --weights model.safetensors --vocab vocab.txt [--model tdt-ctc-110m] [--lower] [--skip-empty]
                                         [input.txt (default: stdin)] [-o output.txt (default: stdout)]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]


def convert(model, lines, out, lower=False, skip_empty=False):
    """Writes one id line per text line -> (lines written, tokens written)."""
    n_lines = n_tok = 0
    for line in lines:
        text = line.strip()
        if lower:
            text = text.lower()
        ids = model.tokenize(text) if text else []
        if skip_empty and not ids:
            continue
        out.write(" ".join(str(i) for i in ids) + "\n")
        n_lines += 1
        n_tok += len(ids)
    return n_lines, n_tok


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("input", nargs="?", help="text file, one sentence per line (default: stdin)")
    ap.add_argument("-o", "--output", help="id file (default: stdout)")
    ap.add_argument("--weights", required=True)
    ap.add_argument("--vocab", required=True)
    ap.add_argument("--model", default="tdt-ctc-110m", help="configuration preset of the weights")
    ap.add_argument("--lower", action="store_true", help="lower-case the text first")
    ap.add_argument("--skip-empty", action="store_true")
    a = ap.parse_args()
    import pkload
    pk = pkload.load()
    from parakeet_cpp_amd import capi
    if a.model not in pk.PRESETS:
        sys.exit(f"unknown --model {a.model}: one of {sorted(pk.PRESETS)}")
    model = capi.Model(a.weights, pk.PRESETS[a.model](), vocab_path=a.vocab)
    src = open(a.input, encoding="utf-8") if a.input else sys.stdin
    dst = open(a.output, "w", encoding="utf-8") if a.output else sys.stdout
    try:
        n_lines, n_tok = convert(model, src, dst, a.lower, a.skip_empty)
    finally:
        if a.input:
            src.close()
        if a.output:
            dst.close()
        model.close()
    print(f"{n_lines} lines, {n_tok} tokens", file=sys.stderr)


if __name__ == "__main__":
    main()
