// parakeet.cpp_amd/csrc/kernels/ngram_lm_dev.hpp -- the n-gram LM lookup of the fused searches (ctc_beam.hip, tdt_beam.hip).
#pragma once
#include "kernels.hpp"

namespace pk {

// lookup(s, c) of ngram_lm.hpp on the device arrays: one 16-byte state record per back-off level, a binary search over its sorted arc
// tokens, one 8-byte arc record; the dense table of the empty context ends the chain.  c < V and m.U <= V (checked by the host).
__device__ __forceinline__ float beam_lm_lookup(const LmDev &m, int s, int c, int &next) {
    float acc = 0.0f;
    while (s != 0) {
        const int4 st = m.state[s];
        int lo = st.x, hi = st.x + st.y, found = -1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1, t = m.arc_tok[mid];
            if (t == c) { found = mid; break; }
            if (t < c) lo = mid + 1; else hi = mid;
        }
        if (found >= 0) {
            const int2 ar = m.arc[found];
            next = ar.y;
            return __fadd_rn(acc, __int_as_float(ar.x));
        }
        acc = __fadd_rn(acc, __int_as_float(st.z));
        s = st.w;
    }
    int2 ar = make_int2(__float_as_int(m.unk_lp), 0);
    if (c < m.U) ar = m.uni[c];
    next = ar.y;
    return __fadd_rn(acc, __int_as_float(ar.x));
}

}  // namespace pk
