"""What the IMM3_INT_IN suites share (test_int_in_host.py, test_gpu_int_in.py, test_gpu_zz_perf_int_in.py): the reference (np.isin over
the same rows), the probe table's hash restated in Python, the lists that are hard for it, and the fuzz's statement generator.  No
threshold is written down here: the forms' bounds come from the library's own imm3_plan_int_list_form."""
import numpy as np

from immutable3_amd import native
from str_range_util import bitmap_words  # noqa: F401  (the batch-major bitmap of a row mask)

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
GOLDEN = 0x9E3779B1


def isin(col, values):
    """bool[n]: exact integer membership (no narrowing: 300 is no member of an int8 column's rows)"""
    return np.isin(np.asarray(col).astype(np.int64), np.array(sorted(set(int(v) for v in values)), dtype=np.int64))


def slots_for(n):
    s = 16
    while s < 2 * n:
        s *= 2
    return s


def home(v, slots):
    """the home slot: the top log2(slots) bits of (uint32)v * 0x9E3779B1"""
    return (((int(v) & 0xFFFFFFFF) * GOLDEN) & 0xFFFFFFFF) >> (32 - (slots.bit_length() - 1))


def same_home_values(n, start=1000):
    """n int32 values that share ONE home slot in the table a list of n values gets"""
    slots = slots_for(n)
    want, out, v = home(start, slots), [], start
    while len(out) < n:
        if home(v, slots) == want:
            out.append(v)
        v += 1
    return out


def lds_largest_n():
    """the largest n whose folded list on an int32 column takes the LDS form (bisection over imm3_plan_int_list_form)"""
    assert native.plan_int_list_form(4, 9) == native.INT_LIST_LDS or native.plan_int_list_form(4, 9) == native.INT_LIST_GLOBAL
    lo, hi = 8, native.INT_IN_MAX_VALUES          # form(lo) < GLOBAL <= form(hi)
    assert native.plan_int_list_form(4, hi) == native.INT_LIST_GLOBAL
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if native.plan_int_list_form(4, mid) == native.INT_LIST_GLOBAL:
            hi = mid
        else:
            lo = mid
    return lo


def args_largest_n():
    n = 0
    while native.plan_int_list_form(4, n + 1) == native.INT_LIST_ARGS:
        n += 1
    return n


def probe_py(slots, empty, max_probe, v):
    """the bounded probe, restated"""
    if v == empty:
        return False
    n = len(slots)
    h = home(v, n)
    for i in range(max_probe):
        x = int(slots[(h + i) & (n - 1)])
        if x == v:
            return True
        if x == empty:
            return False
    return False


# ---- the fuzz: statements over small random tables (drawn on the CPU; test_int_in_host.py holds the generator's refusal rate) ----
class Statement:
    """segments: [(rows, block_rows)]; cols: per segment (id int32[], age int8[], code uint8[n, 4]); leaves: [(column name, kind,
    operand)] with kind in {"in", "gt", "lt", "eq", "match"}; a conjunction"""

    def __init__(self, segments, cols, leaves, limit):
        self.segments, self.cols, self.leaves, self.limit = segments, cols, leaves, limit


COLS = ("id", "age", "code")
CODES = [b"aaaa", b"abcd", b"zzzz", b"m\x00\xff\x80", b"qrst"]


def draw_statement(rng):
    n_seg = int(rng.integers(1, 5))
    segments, cols = [], []
    for _ in range(n_seg):
        n = int(rng.integers(1, 3001))
        segments.append((n, [1024] * (n // 1024) + ([n % 1024] if n % 1024 else [])))
        span = int(rng.choice([4, 60, 5000]))
        ids = rng.integers(-span, span, size=n).astype(np.int32)
        if rng.random() < 0.3:
            ids = np.sort(ids)
        age = rng.integers(-128, 128, size=n).astype(np.int8)
        code = np.frombuffer(b"".join(CODES[int(k)] for k in rng.integers(0, len(CODES), size=n)), dtype=np.uint8).reshape(n, 4).copy()
        cols.append((ids, age, code))
    leaves = []
    for _ in range(int(rng.integers(1, 3))):       # one or two lists
        name = "id" if rng.random() < 0.6 else "age"
        ci = COLS.index(name)
        k = int(rng.integers(0, 41))
        present = np.concatenate([c[ci] for c in cols]).astype(np.int64)
        vals = []
        for _ in range(k):
            if rng.random() < 0.5:
                vals.append(int(present[int(rng.integers(0, present.size))]))
            else:
                vals.append(int(rng.choice([INT32_MIN, INT32_MAX, -129, 128, 300, int(rng.integers(-6000, 6000))])))
        leaves.append((name, "in", vals))
    for _ in range(int(rng.integers(0, 3))):       # further range / Match leaves
        r = rng.random()
        if r < 0.4:
            leaves.append(("id", str(rng.choice(["gt", "lt", "eq"])), float(rng.integers(-70, 70))))
        elif r < 0.8:
            leaves.append(("age", str(rng.choice(["gt", "lt"])), float(rng.integers(-130, 130))))
        else:
            leaves.append(("code", "match", [CODES[int(i)] for i in rng.integers(0, len(CODES), size=int(rng.integers(1, 4)))]))
    order = rng.permutation(len(leaves))
    return Statement(segments, cols, [leaves[int(i)] for i in order], int(rng.choice([0, 0, 1, 7, 100])))


def refused(stmt):
    """a reason the ABI refused such a statement before IMM3_INT_IN existed, or None (this generator draws three columns: none)"""
    return "more than 4 distinct predicate columns" if len({l[0] for l in stmt.leaves}) > 4 else None


def truth(stmt, si):
    """bool[n]: the statement's rows of segment si, in plain numpy"""
    ids, age, code = stmt.cols[si]
    col = {"id": ids.astype(np.int64), "age": age.astype(np.int64)}
    m = np.ones(ids.size, dtype=bool)
    for name, kind, operand in stmt.leaves:
        if kind == "in":
            m &= isin(col[name], operand)
        elif kind == "match":
            m &= np.array([bytes(r) in set(operand) for r in code], dtype=bool)
        else:                                         # the reference narrows a GT / LT / EQ operand to the column's type (d.toByte wraps)
            t = int(operand)
            if name == "age":
                t = (t + 128) % 256 - 128
            m &= (col[name] > t) if kind == "gt" else ((col[name] < t) if kind == "lt" else (col[name] == t))
    return m


def native_sels(stmt, used_names):
    conds = {"in": native.INT_IN, "gt": native.GT, "lt": native.LT, "eq": native.EQ, "match": native.MATCH}
    return [(used_names.index(name), conds[kind], operand) for name, kind, operand in stmt.leaves]
