"""Helpers of the select-tree tests (test_expr_host.py, test_gpu_expr.py, test_gpu_zz_perf_expr.py): trees as nested tuples,
their postfix programs, and the expectation the issue names -- one leaf at a time through the oracle's scan_select, the leaves'
per-batch keep masks combined with numpy & and | as the tree says."""
import numpy as np

from immutable3_amd import native
from oracle import oracle_np

AND, OR = "and", "or"


def postfix(tree):
    """('and' | 'or', left, right) | leaf index  ->  the program of include/imm3.h's select trees"""
    if isinstance(tree, int):
        return [tree]
    op, l, r = tree
    return postfix(l) + postfix(r) + [native.EXPR_AND if op == AND else native.EXPR_OR]


def combine(tree, leaf_values):
    """the tree over per-leaf boolean arrays"""
    if isinstance(tree, int):
        return leaf_values[tree]
    op, l, r = tree
    a, b = combine(l, leaf_values), combine(r, leaf_values)
    return (a & b) if op == AND else (a | b)


def has_or(tree):
    return not isinstance(tree, int) and (tree[0] == OR or has_or(tree[1]) or has_or(tree[2]))


def random_tree(rng, n_leaves):
    """a random binary tree over leaves 0 .. n_leaves - 1, each used once"""
    nodes = list(range(n_leaves))
    while len(nodes) > 1:
        i = int(rng.integers(0, len(nodes) - 1))
        l = nodes.pop(i)
        r = nodes.pop(i)
        nodes.insert(i, (OR if rng.random() < 0.5 else AND, l, r))
    return nodes[0]


def expected_masks(cols, leaves, tree, block_size=1024):
    """per-batch keep masks of the tree over RawColumn-like columns (used-column order)"""
    npcols = [c.npcol() for c in cols]
    per_leaf = [oracle_np.scan_select(npcols, [leaf], block_size)[2] for leaf in leaves]
    n_batches = len(per_leaf[0]) if per_leaf else 0
    return [combine(tree, [pl[k] for pl in per_leaf]) for k in range(n_batches)]


def words_of_masks(masks):
    """the batch-major bitmap: every batch's mask packed little-endian from a fresh word (as scan_select packs them)"""
    words = []
    for keep in masks:
        nw = -(-keep.size // 64)
        padded = np.zeros(nw * 64, np.uint8)
        padded[: keep.size] = keep
        words.append(np.packbits(padded, bitorder="little").view("<u8"))
    return np.concatenate(words).astype(np.uint64) if words else np.zeros(0, np.uint64)
