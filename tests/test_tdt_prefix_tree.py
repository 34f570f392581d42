"""CPU: the prefix-tree builder of the shared TDT total (pk_diag_tdt_prefix_tree) -- host arithmetic, no device."""
import numpy as np
import pytest

from parakeet_cpp_amd import capi

# (strings, clip_of or None, n_clips): duplicates, a prefix of another string, empty strings, a clip without a string, shuffled clip_of
SETS = {
    "one_each": ([[1, 2, 3], [4], []], None, 3),
    "shared_prefixes": ([[1, 2, 3], [1, 2, 4], [1, 5], [2, 1]], [0, 0, 0, 0], 1),
    "duplicates_and_prefix": ([[7, 7, 7], [7, 7], [7, 7, 7], [], [7]], [0, 0, 0, 0, 0], 1),
    "clip_without_a_string": ([[1, 2], [1, 3], [9]], [0, 0, 2], 3),
    "shuffled_clip_of": ([[3, 1], [1, 2, 3], [3, 1, 4], [1, 2], [], [1, 2, 3], [5]], [2, 0, 2, 0, 1, 0, 2], 4),
    "same_tokens_other_clip": ([[1, 2], [1, 2], [1, 2, 3]], [1, 0, 1], 2),
}


@pytest.mark.parametrize("name", list(SETS))
def test_prefix_tree_spells_every_string_and_has_one_node_per_distinct_prefix(name):
    ids, clip_of, n_clips = SETS[name]
    node_off, parent, token, end = capi.tdt_prefix_tree(ids, clip_of, n_clips)
    cl = list(range(len(ids))) if clip_of is None else clip_of
    assert node_off[0] == 0 and len(node_off) == n_clips + 1 and len(parent) == len(token) == node_off[-1]
    for c in range(n_clips):
        p = parent[node_off[c]:node_off[c + 1]]
        assert p[0] == -1 and all(0 <= p[k] < k for k in range(1, len(p))), (c, p)
    for h, s in enumerate(ids):
        base, k, spelled = node_off[cl[h]], end[h], []
        assert 0 <= k < node_off[cl[h] + 1] - base
        while k != 0:
            spelled.append(int(token[base + k]))
            k = parent[base + k]
        assert spelled[::-1] == list(s), (h, spelled[::-1], s)
    prefixes = {(c, ()) for c in range(n_clips)} | {(cl[h], tuple(s[:u])) for h, s in enumerate(ids) for u in range(1, len(s) + 1)}
    assert node_off[-1] == len(prefixes)
    for h, s in enumerate(ids):                                    # equal strings of one clip end at the same node
        for g, r in enumerate(ids):
            if cl[g] == cl[h]:
                assert (end[g] == end[h]) == (list(r) == list(s)), (g, h)


def test_bad_arguments_are_refused_without_a_device():
    with pytest.raises(capi.PkError) as e:
        capi.tdt_prefix_tree([[1], [2]], [0, 3], 2)
    assert e.value.code == -1
    with pytest.raises(capi.PkError) as e:
        capi.tdt_prefix_tree([[1], [2]], None, 3)
    assert e.value.code == -1


@pytest.mark.parametrize("parent,end,dur,code", [([-1, 0, 2], [1], [0, 1], -1), ([-1, 0, 0], [3], [0, 1], -1), ([0, 0, 1], [1], [0, 1], -1),
                                                 ([-1] + [0] * 1536, [5], [0, 1], -7), ([-1, 0, 1], [2], [0, 9], -7)],
                         ids=["parent_not_below", "end_node_outside", "root_with_parent", "1537_nodes", "duration_9"])
def test_tree_walk_refuses_before_it_looks_for_a_device(parent, end, dur, code):
    n = len(parent)
    lat = (np.zeros((1, n - 1), np.float32), np.zeros((1, n), np.float32), np.zeros((1, n, len(dur)), np.float32))
    with pytest.raises(capi.PkError) as e:
        capi.tdt_total_tree([lat], [parent], end, dur)
    assert e.value.code == code
