"""Helpers of the NOT tests (test_expr_not_host.py, test_gpu_expr_not.py): expr_util's trees with one more node, ('not', subtree).
The expectation stays numpy's: each leaf's per-batch keep mask from the oracle's scan_select, combined with &, | and ~ as the tree
says -- ~ of a keep mask of batch.size entries is already confined to the batch's valid rows."""
import numpy as np

from expr_util import AND, OR, words_of_masks  # noqa: F401  (re-exported)
from immutable3_amd import native
from oracle import oracle_np

NOT = "not"


def postfix(tree):
    """('and' | 'or', left, right) | ('not', subtree) | leaf index  ->  the program of include/imm3.h's select trees"""
    if isinstance(tree, int):
        return [tree]
    if tree[0] == NOT:
        return postfix(tree[1]) + [native.EXPR_NOT]
    op, l, r = tree
    return postfix(l) + postfix(r) + [native.EXPR_AND if op == AND else native.EXPR_OR]


def combine(tree, leaf_values):
    """the tree over per-leaf boolean arrays"""
    if isinstance(tree, int):
        return leaf_values[tree]
    if tree[0] == NOT:
        return ~combine(tree[1], leaf_values)
    op, l, r = tree
    a, b = combine(l, leaf_values), combine(r, leaf_values)
    return (a & b) if op == AND else (a | b)


def random_tree(rng, n_leaves, p_not=0.3):
    """a random tree over leaves 0 .. n_leaves - 1, each used once: every binary node AND or OR, and every node (leaves and the
    root included) wrapped in a NOT with probability p_not"""
    def maybe_not(t):
        return (NOT, t) if rng.random() < p_not else t

    nodes = [maybe_not(i) for i in range(n_leaves)]
    while len(nodes) > 1:
        i = int(rng.integers(0, len(nodes) - 1))
        l = nodes.pop(i)
        r = nodes.pop(i)
        nodes.insert(i, maybe_not((OR if rng.random() < 0.5 else AND, l, r)))
    return nodes[0]


def has_not(tree):
    return not isinstance(tree, int) and (tree[0] == NOT or any(has_not(t) for t in tree[1:]))


def expected_masks(cols, leaves, tree, block_size=1024):
    """per-batch keep masks of the tree over RawColumn-like columns (used-column order)"""
    npcols = [c.npcol() for c in cols]
    per_leaf = [oracle_np.scan_select(npcols, [leaf], block_size)[2] for leaf in leaves]
    n_batches = len(per_leaf[0]) if per_leaf else 0
    return [combine(tree, [np.asarray(pl[k], bool) for pl in per_leaf]) for k in range(n_batches)]
