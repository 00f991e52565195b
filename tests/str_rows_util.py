"""Data for the string-Match suites (test_gpu_str_rows*.py, test_str_rows_host.py): a few dozen distinct strings of one width, among
them rows that differ from an IN-list value in exactly one byte at every dword position and rows that share a value's first 16 bytes."""
import numpy as np


def pool_for(rng, width):
    """(pool uint8[k, width], t0, t1): t0 and t1 are the values the IN-lists ask for; the pool also holds, for every dword d of
    the row, t0 with one byte of that dword changed, and (wider than 16 bytes) t0 with only its last byte changed"""
    t0 = rng.integers(97, 123, size=width).astype(np.uint8)
    t1 = rng.integers(97, 123, size=width).astype(np.uint8)
    rows = [t0, t1]
    for d in range(width // 4):
        v = t0.copy()
        v[4 * d + d % 4] ^= 0x01
        rows.append(v)
    last = t0.copy()
    last[-1] ^= 0x02
    rows.append(last)
    first = t1.copy()
    first[0] ^= 0x04
    rows.append(first)
    for _ in range(24):
        rows.append(rng.integers(97, 123, size=width).astype(np.uint8))
    pool = np.unique(np.stack(rows), axis=0)
    return pool[rng.permutation(pool.shape[0])], t0, t1


def make_strings(rng, pool, n):
    return pool[rng.integers(0, pool.shape[0], size=n)].reshape(n, pool.shape[1]).copy()


def in_lists(rng, pool, t0, t1, width):
    """IN-lists of 1, 8, 9 and 40 values, duplicates, values of the wrong length, none at all, and values that are in no row but
    share all but their last byte with one that is"""
    absent = [bytes(rng.integers(65, 91, size=width).astype(np.uint8)) for _ in range(40)]   # upper case: in no row
    near = t0.copy()
    near[-1] ^= 0x40
    p = [bytes(x) for x in pool]
    return [
        [bytes(t0)],
        [bytes(t0), bytes(t1)] + p[:3] + absent[:3],
        [bytes(t0), bytes(t1)] + p[:4] + absent[:3],
        absent[:15] + p[:12] + [bytes(t1)] + absent[15:27],
        [bytes(t0), bytes(t0), bytes(t1), bytes(t0)],
        [bytes(t0)[:-1], bytes(t0) + b"x", bytes(t1)],
        [bytes(t0)[:-1]],
        [],
        [bytes(near)],
        [bytes(near), bytes(t1)],
    ]
