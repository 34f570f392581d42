"""The text of csrc/kernels/: the pieces of the numerics contract that are written once stay written once.  Device code spells the sigma column
permutation as sigma_col() (pk_devmath.h) and stores a product's scalar outputs through gemm_store() (kernels/gemm_epi.hpp); a copy that grows back
fails here.  Host dec_sigma (dec_pack.hpp) and the Python / test spellings are the independent side of the comparisons and are not looked at.  No device."""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "parakeet.cpp_amd", "csrc")
KERNELS = os.path.join(CSRC, "kernels")


def kernel_sources():
    paths = sorted(glob.glob(os.path.join(KERNELS, "*.hip")) + glob.glob(os.path.join(KERNELS, "*.hpp")))
    assert os.path.join(KERNELS, "gemm_epi.hpp") in paths and os.path.join(KERNELS, "kernels.hpp") in paths
    return {os.path.basename(p): open(p).read() for p in paths}


def test_sigma_permutation_is_spelled_once_on_the_device():
    src = kernel_sources()
    hits = [(name, no) for name, txt in src.items() for no, line in enumerate(txt.split("\n"), 1) if "& 3) << 2" in line]
    assert len(hits) == 1 and hits[0][0] == "kernels.hpp", hits
    line = src["kernels.hpp"].split("\n")[hits[0][1] - 1]
    assert line.lstrip().startswith("//"), line                  # the comment that documents GemmArgs::sigma_cols
    # the only definitions in csrc/: sigma_col (device) and dec_sigma (host, the other side of the decode comparisons)
    defs = []
    for dirpath, _, files in os.walk(CSRC):
        for f in files:
            if f.endswith((".h", ".hpp", ".hip", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                defs += [(f, m) for m in re.findall(r"int (\w+)\(int \w+\) \{ return \(\w+ & ~15\) \| \(\(\w+ & 3\) << 2\)", txt)]
    assert sorted(defs) == [("dec_pack.hpp", "dec_sigma"), ("pk_devmath.h", "sigma_col")], defs


def test_sigma16_is_gone():
    assert not [name for name, txt in kernel_sources().items() if "sigma16" in txt]
    assert "sigma16" not in open(os.path.join(CSRC, "pk_devmath.h")).read()


def test_remap_store_is_one_device_function():
    hits = [(name, line.strip()) for name, txt in kernel_sources().items() for line in txt.split("\n") if "remap_gs +" in line]
    code = [h for h in hits if not h[1].startswith("//")]
    assert len(code) == 1 and code[0][0] == "gemm_epi.hpp", hits
    txt = kernel_sources()["gemm_epi.hpp"]
    body = txt[txt.index("void gemm_store("):]
    body = body[: body.index("\n}\n")]
    assert "remap_gs +" in body and "sigma_col(col)" in body   # the remap store and the sigma-column store sit in gemm_store
