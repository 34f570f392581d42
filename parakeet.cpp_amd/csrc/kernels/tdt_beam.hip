// parakeet.cpp_amd/csrc/kernels/tdt_beam.hip -- TDT beam search with n-best output on the device.
//
// The specification is tests/tdt_beam_ref.py: a max-path search over the lattice of section 5.5.2, every value compared bit for bit.  The
// rows are R = B W virtual utterances, beam slot w of clip b is row b W + w.  The host (tdt_beam.cpp) enqueues per step: the gather below, one
// prediction-net step over all rows on the decode loop's skinny products, the activation below, the heads product, the expansion, the pruning.
// The beam lives in two copies, step s reads copy s & 1 and writes the other; a clip without a live hypothesis keeps its beam where its last
// step left it (steps_done[b] tells the back-trace which copy) and every kernel here returns at once for it.  No kernel waits on another.
//
//   tdt_beam_init_kernel     the start state: slot 0 of every clip holds the empty prefix at t = 0 with score 0; every row is marked as born
//       from a label arc with the blank as its token, so the first step's prediction-net step consumes [blank] from the zero state.
//   tdt_beam_gather_kernel   one workgroup per row: h, c (every LSTM layer) and pred_proj of the row's parent.  The parent's state is what
//       the prediction-net step of the step before computed when the parent was born from a label arc, else what that step gathered.
//   tdt_beam_act_kernel      z = relu(enc_proj[t] + pred_proj) of a live row, one wave per row: joint_act_row (tdt_lattice_dev.hpp), the row of
//       tdt_lattice_act_kernel, with the clip's row offset and the row's own frame pointer.
//   tdt_beam_expand_kernel   one wave per live row of the heads product's output [V + D]: the canonical log-softmax (decode_dev.hpp
//       wave_row_max_lse, wave_logsoftmax_low8: what tdt_lattice_keep_kernel takes), then the K best non-blank labels by (log-prob down,
//       id up) -- every lane keeps the best of its strided elements, a round is one wave argmax and a rescan by the winning lane alone --, the blank inserted by the same order, the
//       duration head's ranks, and the candidate scores s + (x + dl) in the order label rank, duration rank.
//   tdt_beam_prune_kernel    one workgroup of 256 threads per clip.  The pool (finished hypotheses at positions w, the candidate c of slot
//       w at W + w C + c, C = (K + 1) Kd) is an LDS array of 64-bit keys (order-preserving score bits, then position inverted); a round
//       takes the block's largest key, and the entry joins the new beam unless an entry chosen before it is the same (prefix, t).  Keys
//       come out in (score down, position up) order, so of a group of equal states the first one out is the one the specification keeps.
//       Prefix equality: frame, length and a 64-bit hash first, then the token arrays themselves, all threads comparing a stride each.
//       Writes the new beam, its token arrays and one back-pointer record per slot.
//   tdt_beam_trace_kernel    one thread per returned hypothesis: walks the records from the clip's last step back to step 0.
//
// Limits (host side: tdt_beam.cpp refuses with PK_ERR_UNSUPPORTED before anything is allocated): W <= 16, K <= 16, Kd <= 8, D <= 8,
// scratch of a call <= 1 GiB.  Pool: 16 + 16 x 17 x 8 = 2192 keys = 17536 bytes of LDS.
//
// Code objects (hipcc -O3 --offload-arch=gfx950, from the .s of -save-temps):
//   tdt_beam_expand_kernel   43 VGPR 50 SGPR  LDS     0 B  scratch 0 B; 0 VGPR spills, 0 SGPR spills
//   tdt_beam_prune_kernel    60 VGPR 85 SGPR  LDS 18784 B  scratch 0 B; 0 VGPR spills, 0 SGPR spills
//   tdt_beam_gather_kernel   19 VGPR 31 SGPR, tdt_beam_act_kernel 46 VGPR 17 SGPR, tdt_beam_trace_kernel 27 VGPR 35 SGPR, tdt_beam_init_kernel 23 VGPR
//   36 SGPR: no LDS, no scratch, no spills
//
// With n-gram LM shallow fusion (the specification is tests/tdt_beam_lm_ref.py): init, expand, prune and trace are
// templates on kLm, and the <false> instantiations are the kernels above, instruction for instruction (their figures did not move); the
// launchers take the <true> ones when TdtBeamDev::lmstate is set.  A beam slot carries two more words, the LM automaton's state after its
// prefix and the prefix's LM score.  The fused expand: after the K + 1 labels are sorted, lane i <= K that holds a non-blank id runs
// beam_lm_lookup (ngram_lm_dev.hpp, the fused CTC walk's) -- at most 16 lanes of the wave walk the automaton side by side, the row pays the
// longest chain once -- and stores lm2 = lm + ((alpha * lp) + beta) and the next state beside the label; the blank's entry holds the row's
// own.  The fused prune builds its keys from f = score + lm (a finished entry's own two values, a candidate's cand + lm2 of its label), so
// duplicates and the W best are decided by f; score, lm and the state of a chosen entry go to the new beam.  The fused trace writes lm_score.
//   tdt_beam_expand_kernel<true>  41 VGPR 70 SGPR  LDS     0 B  scratch 0 B; 0 VGPR spills, 0 SGPR spills
//   tdt_beam_prune_kernel<true>   68 VGPR 86 SGPR  LDS 19040 B  scratch 0 B; 0 VGPR spills, 0 SGPR spills
//   tdt_beam_init_kernel<true> 28 VGPR 42 SGPR, tdt_beam_trace_kernel<true> 27 VGPR 35 SGPR: no LDS, no scratch, no spills
#include "decode_dev.hpp"
#include "tdt_lattice_dev.hpp"
#include "ngram_lm_dev.hpp"

namespace pk {

namespace {

constexpr int kPool = kTdtBeamMaxWidth + kTdtBeamMaxWidth * (kTdtBeamMaxLabels + 1) * kTdtBeamMaxDurs;
typedef unsigned long long u64;

// bits of a float whose unsigned order is the float order (-inf lowest)
__device__ __forceinline__ unsigned ord_bits(float f) {
    const unsigned u = (unsigned)__float_as_int(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ u64 pool_key(float score, int pos) { return ((u64)ord_bits(score) << 32) | (u64)(0xFFFFFFFFu - (unsigned)pos); }
__device__ __forceinline__ u64 hash_push(u64 h, int tok) { return (h ^ (u64)(unsigned)(tok + 1)) * 0x100000001B3ull + 0x9E3779B97F4A7C15ull; }

}  // namespace

template <bool kLm>
__global__ __launch_bounds__(256) void tdt_beam_init_kernel(TdtBeamDev a) {
    const int r = blockIdx.x * 256 + threadIdx.x, R = a.B * a.W;
    if (r < R) {
        const bool first = r % a.W == 0;
        for (int p = 0; p < 2; ++p) {
            const int i = p * R + r;
            a.valid[i] = p == 0 && first; a.t[i] = 0; a.len[i] = 0; a.par[i] = r; a.born[i] = p == 0; a.tok[i] = a.blank;
            a.score[i] = p == 0 && first ? 0.0f : -__builtin_huge_valf(); a.hash[i] = 0;
            if constexpr (kLm) { a.lmstate[i] = a.ngram.start; a.lm[i] = 0.0f; }
        }
    }
    if (r < a.B) { a.live[r] = 1; a.steps_done[r] = 0; }
    if (r == 0) a.live_total[0] = a.B;
}

__global__ __launch_bounds__(256) void tdt_beam_gather_kernel(TdtBeamDev a, int s) {
    const int r = blockIdx.x, R = a.B * a.W, b = r / a.W;
    if (!a.live[b]) return;
    const int p = s & 1, q = p ^ 1;
    const int src = a.par[p * R + r];
    const bool fresh = a.born[q * R + src] != 0;                     // the parent's own birth: its state is the prediction-net step's output
    const float *hs = fresh ? a.hN : a.hG[q], *cs = fresh ? a.cN : a.cG[q], *ps = fresh ? a.ppN : a.ppG[q];
    float *hd = a.hG[p], *cd = a.cG[p], *pd = a.ppG[p];
    for (int l = 0; l < a.L; ++l) {
        const int64_t so = ((int64_t)l * R + src) * a.Hp, d0 = ((int64_t)l * R + r) * a.Hp;
        for (int j = threadIdx.x; j < a.Hp; j += 256) { hd[d0 + j] = hs[so + j]; cd[d0 + j] = cs[so + j]; }
    }
    for (int j = threadIdx.x; j < a.J; j += 256) pd[(int64_t)r * a.J + j] = ps[(int64_t)src * a.J + j];
}

__global__ __launch_bounds__(256) void tdt_beam_act_kernel(TdtBeamDev a, int s, const float *__restrict__ ep, float *__restrict__ z) {
    const int lane = threadIdx.x & 63, R = a.B * a.W;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int b = r / a.W, p = s & 1;
    if (!a.live[b]) return;
    const int T = a.T[b], t = a.t[p * R + r];
    if (!a.valid[p * R + r] || t >= T) return;
    const int J = a.J;
    joint_act_row(ep + ((int64_t)a.row0[b] + t) * J, (a.born[p * R + r] ? a.ppN : a.ppG[p]) + (int64_t)r * J, z + (int64_t)r * J, J, lane);
}

template <bool kLm>
__global__ __launch_bounds__(256) void tdt_beam_expand_kernel(TdtBeamDev a, int s, const float *__restrict__ logits) {
    const int lane = threadIdx.x & 63, R = a.B * a.W;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int b = r / a.W, p = s & 1;
    if (!a.live[b]) return;
    if (!a.valid[p * R + r] || a.t[p * R + r] >= a.T[b]) return;
    const int V = a.V, D = a.D, K = a.K, Kd = a.Kd, blank = a.blank;
    const float NEG = -__builtin_huge_valf();
    const float *x = logits + (int64_t)r * (V + D);
    const RowLse rl = wave_row_max_lse(x, V, lane);
    const float m = rl.m, lse = rl.lse;
    const float lb = (x[blank] - m) - lse;
    const int di = lane & 7;
    const float dlv = wave_logsoftmax_low8(x + V, D, lane);         // the duration head: lane l holds the log-prob of index l & 7
    int rank = 0;
    for (int j = 0; j < D; ++j) {
        const float o = __shfl(dlv, j);
        rank += (o > dlv || (o == dlv && j < di)) ? 1 : 0;
    }
    float sdv = NEG;                                                // lane q < Kd: the duration log-prob of rank q
    for (int j = 0; j < D; ++j) {
        const int rj = __shfl(rank, j);
        const float vj = __shfl(dlv, j);
        if (lane == rj) sdv = vj;
    }
    if (lane < D && rank < Kd) { a.dur_i[(int64_t)r * Kd + rank] = lane; a.dur_lp[(int64_t)r * Kd + rank] = dlv; }
    // the K best non-blank labels: mine = the best of this lane's elements that comes after the last pick in (log-prob down, id up) order
    auto scan = [&](float pl, int pi) {
        float best = NEG;
        int bi = 0x7fffffff;
        for (int i = lane; i < V; i += 64) {
            const float l = (x[i] - m) - lse;
            const bool after = l < pl || (l == pl && i > pi);
            if (i != blank && after && (bi == 0x7fffffff || l > best)) { best = l; bi = i; }
        }
        return BestLP{best, bi};
    };
    BestLP mine = scan(__builtin_huge_valf(), -1);
    float plp = NEG;                                                // lane k < K: the k-th pick
    int pid = -1;
    for (int k = 0; k < K; ++k) {
        float best = mine.lp;
        int bi = mine.idx;
        wave_butterfly([&](auto off) {
            const float ob = wave_xor<decltype(off)::value>(best);
            const int oi = wave_xor_i<decltype(off)::value>(bi);
            if (oi != 0x7fffffff && (bi == 0x7fffffff || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
        });
        if (bi == 0x7fffffff) break;                                // (wave-uniform: fewer than K comparable labels)
        if (lane == k) { plp = best; pid = bi; }
        if ((bi & 63) == lane) mine = scan(best, bi);
    }
    // the blank joins the sorted picks by the same order
    const bool before = lane < K && pid >= 0 && (plp > lb || (plp == lb && pid < blank));
    const int nb = __popcll(__ballot(before));
    const float ulp = __shfl_up(plp, 1);
    const int uid = __shfl_up(pid, 1);
    const float slp = lane < nb ? plp : lane == nb ? lb : ulp;
    const int sid = lane < nb ? pid : lane == nb ? blank : uid;
    if (lane <= K) { a.lab_id[(int64_t)r * (K + 1) + lane] = sid; a.lab_lp[(int64_t)r * (K + 1) + lane] = slp; }
    if constexpr (kLm) {
        // one lookup per label: the lanes of the K labels walk the automaton side by side, the row pays the longest chain once
        if (lane <= K) {
            int ls = a.lmstate[p * R + r];
            float lmv = a.lm[p * R + r];
            if (sid >= 0 && sid != blank) {
                int nx = 0;
                const float lp = beam_lm_lookup(a.ngram, ls, sid, nx);
                lmv = __fadd_rn(lmv, __fadd_rn(__fmul_rn(a.ngram.alpha, lp), a.ngram.beta));    // three roundings, no fma
                ls = nx;
            }
            a.lab_ls[(int64_t)r * (K + 1) + lane] = ls; a.lab_lm[(int64_t)r * (K + 1) + lane] = lmv;
        }
    }
    const float sc = a.score[p * R + r];
    const int C = (K + 1) * Kd;
    for (int c0 = 0; c0 < C; c0 += 64) {
        const int c = c0 + lane, li = c / Kd < K ? c / Kd : K;
        const float xl = __shfl(slp, li), yd = __shfl(sdv, c % Kd);
        if (c < C) a.cand[(int64_t)r * C + c] = sc + (xl + yd);
    }
}

template <bool kLm>
__global__ __launch_bounds__(256) void tdt_beam_prune_kernel(TdtBeamDev a, int s) {
    __shared__ u64 key[kPool];
    __shared__ u64 wbest[4];
    __shared__ u64 bh[kTdtBeamMaxWidth], sel_hash[kTdtBeamMaxWidth];
    __shared__ int bv[kTdtBeamMaxWidth], bt[kTdtBeamMaxWidth], bl[kTdtBeamMaxWidth];
    __shared__ float bs[kTdtBeamMaxWidth];
    __shared__ int sel_w[kTdtBeamMaxWidth], sel_tok[kTdtBeamMaxWidth], sel_t[kTdtBeamMaxWidth], sel_len[kTdtBeamMaxWidth], sel_rec[kTdtBeamMaxWidth];
    __shared__ float sel_score[kTdtBeamMaxWidth], sel_lp[kTdtBeamMaxWidth];
    __shared__ float blm[kTdtBeamMaxWidth], sel_lm[kTdtBeamMaxWidth];         // (kLm only: the unfused kernel never names them)
    __shared__ int bls[kTdtBeamMaxWidth], sel_ls[kTdtBeamMaxWidth];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    if (!a.live[b]) return;
    const int W = a.W, K = a.K, Kd = a.Kd, R = a.B * W, MT = a.max_tokens, blank = a.blank;
    const int p = s & 1, q = p ^ 1, base = b * W, T = a.T[b];
    const int C = (K + 1) * Kd, P = W + W * C;
    const int *pre_p = a.prefix + (int64_t)p * R * MT;
    int *pre_q = a.prefix + (int64_t)q * R * MT;
    if (tid < W) {
        const int i = p * R + base + tid;
        bv[tid] = a.valid[i]; bt[tid] = a.t[i]; bl[tid] = a.len[i]; bs[tid] = a.score[i]; bh[tid] = a.hash[i];
        if constexpr (kLm) { blm[tid] = a.lm[i]; bls[tid] = a.lmstate[i]; }
    }
    __syncthreads();
    u64 mybest = 0;
    for (int pos = tid; pos < P; pos += 256) {
        u64 k = 0;
        if (pos < W) {
            if (bv[pos] && bt[pos] >= T) k = pool_key(kLm ? __fadd_rn(bs[pos], blm[pos]) : bs[pos], pos);
        } else {
            const int w = (pos - W) / C, c = (pos - W) - w * C;
            if (bv[w] && bt[w] < T) {
                const int id = a.lab_id[(int64_t)(base + w) * (K + 1) + c / Kd];
                if (id >= 0 && (id == blank || bl[w] < MT)) {
                    float f = a.cand[(int64_t)(base + w) * C + c];
                    if constexpr (kLm) f = __fadd_rn(f, a.lab_lm[(int64_t)(base + w) * (K + 1) + c / Kd]);      // the keys order by f = score + lm
                    k = pool_key(f, pos);
                }
            }
        }
        key[pos] = k;
        mybest = k > mybest ? k : mybest;
    }
    __syncthreads();
    int nsel = 0;
    while (nsel < W) {
        u64 v = mybest;
        for (int off = 32; off >= 1; off >>= 1) {
            const u64 o = __shfl_xor(v, off);
            v = o > v ? o : v;
        }
        if (lane == 0) wbest[tid >> 6] = v;
        __syncthreads();
        v = wbest[0];
        for (int i = 1; i < 4; ++i) v = wbest[i] > v ? wbest[i] : v;
        if (v == 0) break;                                          // (block-uniform: the pool is used up)
        const int pos = (int)(0xFFFFFFFFu - (unsigned)v);
        // what the entry is
        int w, tok = -1, rec = 0, tn, ln;
        float lp = 0.0f, sc, lmv = 0.0f;
        int lms = 0;
        u64 hn;
        if (pos < W) {
            w = pos; tn = bt[w]; ln = bl[w]; sc = bs[w]; hn = bh[w];
            if constexpr (kLm) { lmv = blm[w]; lms = bls[w]; }
        } else {
            w = (pos - W) / C;
            const int c = (pos - W) - w * C, li = c / Kd, dr = c - li * Kd;
            const int id = a.lab_id[(int64_t)(base + w) * (K + 1) + li], dix = a.dur_i[(int64_t)(base + w) * Kd + dr];
            const int dur = a.durations[dix];
            sc = a.cand[(int64_t)(base + w) * C + c];
            if constexpr (kLm) { lmv = a.lab_lm[(int64_t)(base + w) * (K + 1) + li]; lms = a.lab_ls[(int64_t)(base + w) * (K + 1) + li]; }
            if (id == blank) { tn = bt[w] + (dur > 1 ? dur : 1); ln = bl[w]; hn = bh[w]; }
            else {
                tok = id; lp = a.lab_lp[(int64_t)(base + w) * (K + 1) + li]; rec = bt[w] * 8 + dix;
                tn = bt[w] + dur; ln = bl[w] + 1; hn = hash_push(bh[w], id);
            }
            tn = tn < T ? tn : T;
        }
        bool dup = false;
        for (int j = 0; j < nsel && !dup; ++j) {
            if (sel_t[j] != tn || sel_len[j] != ln || sel_hash[j] != hn) continue;
            const int w2 = sel_w[j], tok2 = sel_tok[j];
            if (w2 == w) { dup = tok2 == tok; continue; }
            // the token strings themselves: element i of an entry is its parent's token i, then the token it appends
            int differ = 0;
            for (int i = tid; i < ln; i += 256) {
                const int x1 = i < bl[w] ? pre_p[(int64_t)(base + w) * MT + i] : tok;
                const int x2 = i < bl[w2] ? pre_p[(int64_t)(base + w2) * MT + i] : tok2;
                differ |= x1 != x2;
            }
            dup = !__syncthreads_or(differ);
        }
        if (tid == 0) {
            key[pos] = 0;
            if (!dup) {
                sel_w[nsel] = w; sel_tok[nsel] = tok; sel_t[nsel] = tn; sel_len[nsel] = ln; sel_hash[nsel] = hn; sel_score[nsel] = sc;
                sel_lp[nsel] = lp; sel_rec[nsel] = rec;
                if constexpr (kLm) { sel_lm[nsel] = lmv; sel_ls[nsel] = lms; }
            }
        }
        __syncthreads();
        if ((pos & 255) == tid) {
            mybest = 0;
            for (int i = tid; i < P; i += 256) mybest = key[i] > mybest ? key[i] : mybest;
        }
        if (!dup) ++nsel;
    }
    __syncthreads();
    // the new beam
    for (int j = 0; j < nsel; ++j) {
        const int w = sel_w[j], n = bl[w];
        for (int i = tid; i < n; i += 256) pre_q[(int64_t)(base + j) * MT + i] = pre_p[(int64_t)(base + w) * MT + i];
        if (tid == 0 && sel_tok[j] >= 0) pre_q[(int64_t)(base + j) * MT + n] = sel_tok[j];      // (n < max_tokens: a full hypothesis forms no label candidate)
    }
    if (tid < W) {
        const int i = q * R + base + tid;
        const bool on = tid < nsel;
        a.valid[i] = on; a.t[i] = on ? sel_t[tid] : 0; a.len[i] = on ? sel_len[tid] : 0; a.score[i] = on ? sel_score[tid] : -__builtin_huge_valf();
        a.hash[i] = on ? sel_hash[tid] : 0; a.par[i] = base + (on ? sel_w[tid] : tid); a.born[i] = on && sel_tok[tid] >= 0;
        a.tok[i] = on && sel_tok[tid] >= 0 ? sel_tok[tid] : blank;
        if constexpr (kLm) { a.lm[i] = on ? sel_lm[tid] : 0.0f; a.lmstate[i] = on ? sel_ls[tid] : 0; }
        a.bp[(int64_t)s * R + base + tid] = make_int4(on ? sel_w[tid] : tid, on ? sel_tok[tid] : -1, on ? sel_rec[tid] : 0, on ? __float_as_int(sel_lp[tid]) : 0);
    }
    if (tid == 0) {
        int n_live = 0;
        for (int j = 0; j < nsel; ++j) n_live += sel_t[j] < T ? 1 : 0;
        a.live[b] = n_live; a.steps_done[b] = s + 1;
        if (n_live) atomicAdd(a.live_total + s + 1, n_live);
    }
}

template <bool kLm>
__global__ __launch_bounds__(64) void tdt_beam_trace_kernel(TdtBeamDev a, TdtBeamOut o) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.B * a.N) return;
    const int b = i / a.N, n = i - b * a.N, W = a.W, R = a.B * W, MT = a.max_tokens, T = a.T[b];
    const int steps = a.steps_done[b], p = steps & 1, base = b * W;
    int slot = -1, seen = 0, any = 0;
    for (int w = 0; w < W; ++w) {
        if (a.valid[p * R + base + w] && a.t[p * R + base + w] >= T) {
            any = 1;
            if (seen == n && slot < 0) slot = w;
            ++seen;
        }
    }
    if (n == 0) o.ok[b] = any;
    if constexpr (kLm) o.lm_score[i] = slot < 0 ? 0.0f : a.lm[p * R + base + slot];
    if (slot < 0) { o.lens[i] = 0; o.score[i] = -__builtin_huge_valf(); return; }        // (the token arrays are zero-filled by the host)
    int u = a.len[p * R + base + slot];
    o.lens[i] = u; o.score[i] = a.score[p * R + base + slot];
    const int64_t o0 = (int64_t)i * MT;
    for (int st = steps - 1; st >= 0 && u > 0; --st) {
        const int4 rec = a.bp[(int64_t)st * R + base + slot];
        if (rec.y >= 0) {
            --u;
            const int t = rec.z >> 3, dix = rec.z & 7;
            o.ids[o0 + u] = rec.y; o.start[o0 + u] = t; o.end[o0 + u] = tdt_token_end(t, a.durations[dix], T); o.dur_idx[o0 + u] = dix;
            o.conf[o0 + u] = dexpf(__int_as_float(rec.w));
        }
        slot = rec.x;
    }
}

void launch_tdt_beam_init(const TdtBeamDev &a, hipStream_t s) {
    const int n = a.B * a.W;
    if (a.lmstate) hipLaunchKernelGGL(tdt_beam_init_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(tdt_beam_init_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
}
void launch_tdt_beam_gather(const TdtBeamDev &a, int step, hipStream_t s) {
    hipLaunchKernelGGL(tdt_beam_gather_kernel, dim3((unsigned)(a.B * a.W)), dim3(256), 0, s, a, step);
}
void launch_tdt_beam_act(const TdtBeamDev &a, int step, const float *ep, float *z, hipStream_t s) {
    hipLaunchKernelGGL(tdt_beam_act_kernel, dim3((unsigned)((a.B * a.W + 3) / 4)), dim3(256), 0, s, a, step, ep, z);
}
void launch_tdt_beam_expand(const TdtBeamDev &a, int step, const float *logits, hipStream_t s) {
    if (a.lmstate) hipLaunchKernelGGL(tdt_beam_expand_kernel<true>, dim3((unsigned)((a.B * a.W + 3) / 4)), dim3(256), 0, s, a, step, logits);
    else hipLaunchKernelGGL(tdt_beam_expand_kernel<false>, dim3((unsigned)((a.B * a.W + 3) / 4)), dim3(256), 0, s, a, step, logits);
}
void launch_tdt_beam_prune(const TdtBeamDev &a, int step, hipStream_t s) {
    if (a.W < 1 || a.W > kTdtBeamMaxWidth || a.K < 1 || a.K > kTdtBeamMaxLabels || a.Kd < 1 || a.Kd > kTdtBeamMaxDurs || a.D < 1 || a.D > 8 || a.Kd > a.D ||
        a.K > a.V - 1) {
        fprintf(stderr, "parakeet_amd: internal error: launch_tdt_beam_prune outside the kernel's limits (W %d, K %d, Kd %d, D %d)\n", a.W, a.K, a.Kd, a.D);
        abort();
    }
    if (a.lmstate) hipLaunchKernelGGL(tdt_beam_prune_kernel<true>, dim3((unsigned)a.B), dim3(256), 0, s, a, step);
    else hipLaunchKernelGGL(tdt_beam_prune_kernel<false>, dim3((unsigned)a.B), dim3(256), 0, s, a, step);
}
void launch_tdt_beam_trace(const TdtBeamDev &a, const TdtBeamOut &o, hipStream_t s) {
    if (a.lmstate) hipLaunchKernelGGL(tdt_beam_trace_kernel<true>, dim3((unsigned)((a.B * a.N + 63) / 64)), dim3(64), 0, s, a, o);
    else hipLaunchKernelGGL(tdt_beam_trace_kernel<false>, dim3((unsigned)((a.B * a.N + 63) / 64)), dim3(64), 0, s, a, o);
}

}  // namespace pk
