// parakeet.cpp_amd/csrc/tdt_tree.hpp -- host side of the forward-algorithm totals on one prefix tree per clip (kernels/tdt_tree.hip):
// the prefix-tree builder, the plan of a call (groups of whole clips), the tables of a group and its launches.
#pragma once
#include "tdt_align.hpp"

namespace pk {

class Model;

// The prefix trees of a call, packed clip after clip: clip c owns nodes [node_off[c], node_off[c + 1]) -- at least one, node 0 the empty prefix
// (parent -1), parent[k] < k, token[k] on the edge into k -- and hypothesis h ends at the clip-local node end_node[h] of clip clip_of[h].  Two
// equal strings end at the same node; a string that is a prefix of another ends at an inner node; an empty string at node 0.
struct TdtPrefixTree {
    std::vector<int32_t> node_off, parent, token, end_node;
};
// Host only.  clip_of == nullptr: hypothesis h on clip h (n_hyp == n_clips).  Nodes are numbered in the order the strings first reach them.
void tdt_prefix_tree_build(TdtPrefixTree &t, const int32_t *ids, const int32_t *id_offsets, const int32_t *clip_of, int n_clips, int n_hyp);

// Scratch of one group of clips, with cells = sum_c T_c n_c and labs = sum_c T_c (n_c - 1):
//   lattice values   4 (labs + cells (1 + D)) bytes
// and, when the lattice is computed from a model,
//   rows chunk       chunk_rows (V + D + J) 4 bytes      (chunk_rows = tdt_align_chunk_rows(V + D), at most cells; none on the bf16 lattice kernel)
//   prediction net   nodes (J + 1) 4 bytes
// capped at kTdtAlignMaxScratch.  A group is consecutive WHOLE clips (those with a hypothesis), at most kTdtTotalGroupHyps hypotheses unless one clip
// alone has more, as many clips as stay under the cap.  Every value is computed from its own (clip, prefix) rows, so the grouping changes no bit.
struct TdtTreeWs {
    // one group: device buffers, the host images of its tables, sizes
    DevBuf lab, blk, dl, tab, tab64, out, pp, z, logits, h, hn, c, cn;
    std::vector<int32_t> h_tab;                     // every int table of the group, back to back (o_* are their first elements)
    std::vector<int64_t> h_tab64;                   // cell_off[C + 1], lab_off[C + 1]
    size_t o_T = 0, o_node_off = 0, o_row0 = 0, o_parent = 0, o_token = 0, o_ppos = 0, o_child_off = 0, o_child = 0, o_s_node = 0, o_s_parent = 0,
           o_s_depth = 0, o_dstart = 0, o_hyp_off = 0, o_hyp_end = 0, o_tok_d = 0, o_pslot = 0;
    size_t o_child_s = 0, o_child_tok = 0;          // every node's children sorted by token, laid out as o_child: the node and its token (kernels/tdt_tree_bf16.hip)
    std::vector<int32_t> lvl;                       // the group's nodes in depth order (depth, then clip, then node): first entry of every depth, [levels + 1]
    std::vector<int32_t> slot_hyp;                  // result slot (hypotheses grouped by clip) -> hypothesis of the call
    int C = 0, D = 0, n_hyp = 0, nodes = 0, n_max = 0, dur_max = 0, chunk_rows = 0, width = 0;
    int durations[8] = {};
    int64_t cells = 0, labs = 0;
    TdtTree tree() const;                           // device view (after tdt_tree_upload)
    // the arguments of the bf16 lattice kernel over this group, but for the weights (device view)
    TdtTreeLatticeBf16Args lattice_bf16_args(const float *ep, const float *pp, int V, int J, int blank) const;
    // one call of the model entry points
    TdtPrefixTree pt;
    std::vector<int32_t> T_of, row0_of;             // [n_clips]
    std::vector<int32_t> hc_off, hc_list;           // hypotheses by clip (CSR), in the caller's order within a clip
    std::vector<int32_t> walked, gstart;            // clips with a hypothesis, ascending; group g is walked[gstart[g] .. gstart[g + 1])
};

// rows_chunk false: the lattice comes from the one launch of kernels/tdt_tree_bf16.hip (Model::tdt_lattice_bf16), which has no rows chunk
size_t tdt_tree_scratch(int64_t cells, int64_t labs, int64_t nodes, int D, int V, int J, bool rows_chunk = true);
// The limits that do not depend on the tree's shape (D, durations): PK_ERR_UNSUPPORTED.  -> dur_max
int tdt_tree_check_durations(const int32_t *durations, int D);
// Host only: the tables of one group -- clips cl[0 .. C) of a call whose per-clip arrays are T_of / row0_of (row0_of nullptr: a host lattice, no
// prediction net), trees pt (pt.token may be empty then), hypotheses by clip hc_off / hc_list.  Refuses (PK_ERR_UNSUPPORTED) a clip of more than
// kTdtTreeMaxNodes nodes and a group over the cap (rows_chunk as tdt_tree_scratch takes it).
void tdt_tree_stage(TdtTreeWs &ws, const int32_t *cl, int C, const int32_t *T_of, const int32_t *row0_of, const TdtPrefixTree &pt, const int32_t *hc_off,
                    const int32_t *hc_list, const int32_t *durations, int D, int V, int J, int blank, bool rows_chunk = true);
// reserves the group's lattice buffers and uploads its tables on s
void tdt_tree_upload(TdtTreeWs &ws, hipStream_t s);
// pred_proj of every node: one lock-step step per DEPTH on the decode loop's skinny products, every row's (h, c) gathered from its parent's row -> ws.pp
void run_tdt_tree_pred(Model &m, TdtTreeWs &ws, hipStream_t s);
// lab / blk / dl of every (clip, frame, node) from ep = enc_proj of the call's packed frames, in chunks of ws.chunk_rows rows of the fp32 heads product;
// with Model::tdt_lattice_bf16 on, ONE launch of kernels/tdt_tree_bf16.hip over all rows instead (ws.chunk_rows, ws.z and ws.logits unused)
void run_tdt_tree_lattice(Model &m, TdtTreeWs &ws, const float *d_ep, hipStream_t s);
// the walk over ws.lab / blk / dl: results on the device in ws.out (total[n_hyp], ok[n_hyp], by result slot)
void run_tdt_tree_dp(TdtTreeWs &ws, hipStream_t s);
// Plans a call of the model entry points on the tree path (host only; refuses before anything is allocated); the arguments of tdt_total_plan_call.
void tdt_tree_plan_call(Model &m, TdtTreeWs &ws, const int32_t *n_frames, int n_clips, int T, const int32_t *ids, const int32_t *id_offsets,
                        const int32_t *clip_of, int n_hyp);
// Queues the planned call group by group (synchronises once per group); total / ok [n_hyp] by the caller's hypothesis index.  ev / ms as run_tdt_total_call.
void run_tdt_tree_call(Model &m, TdtTreeWs &ws, const float *d_ep, std::vector<float> &total, std::vector<int32_t> &ok, hipEvent_t *ev = nullptr,
                       float *ms = nullptr);
size_t tdt_tree_bytes(const TdtTreeWs &ws);

}  // namespace pk
