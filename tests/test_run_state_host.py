"""CPU checks of tests/run_state_model.py: do the committed sequences cover what they claim to, and does the walker have teeth?

Coverage: for every subject, every getter that applies to it is seen directly behind each of the three run entries, behind a launch of
a graph of each recordable entry, behind a recording that has not been launched, behind a reservation and behind another getter; the
call orders the issue names as suspects are prefixes of committed sequences; and IMM3_ERR_STATE stays the exception (at most a quarter
of a subject's getter steps, never more than six steps in a row), so that a walk spends its steps on values.

Teeth: FakeHandle is a stand-in for native.DeviceQuery that implements the contract from a flag record the way the library does --
run entries set flags, getters settle lazily, a graph saves and restores the record.  The walker must pass it on every committed
sequence, and must fail every one of its mutants -- each a defect this project has had, was suspected of, or was found to have by
the first walk on a device -- on at least one."""
import numpy as np
import pytest

import run_state_model as rsm
from run_state_model import GROUP_COL, Model, StateError, SUBJECTS, SUBJECT_BY_NAME, is_getter, sequences, walk

GARBAGE = 0xA5A5A5A5A5A5A5A5


# ---- the stand-in's data and what is true of it -----------------------------------------------------------------------------------
class FakeTruth:
    """200 rows, every seventh survives; a small limit is met within the first 64 rows (a limit scan's first chunk)."""
    N, CHUNK = 200, 64

    def __init__(self, s):
        self.s = s
        i = np.arange(self.N)
        self.keep = i % 7 == 3
        self.surv = np.flatnonzero(self.keep)
        self.vals = ((i * 37) % 101).astype(np.int32)
        self.count = int(self.keep.sum())
        self.bitmap = self._words(self.keep)
        self.limit = {"": 0, "small": 3, "large": self.count + 7}[s.limit]
        self.stops = s.limit == "small"
        head = self.keep.copy()
        head[self.CHUNK:] = False
        self.prefix_count, self.prefix_bitmap = int(head.sum()), self._words(head)
        # groups: key = row % 5 of the survivors, in first-seen order; aggregates {count, max(vals), min(vals)}
        keys = self.surv % 5
        self.g_keys = np.array(list(dict.fromkeys(keys.tolist())), np.uint64)
        self.g_first = np.array([self.surv[keys == k][0] for k in self.g_keys], np.uint32)
        self.g_counts = np.array([(keys == k).sum() for k in self.g_keys], np.uint64)
        v = self.vals[self.surv]
        self.g_vals = np.array([[(keys == k).sum(), v[keys == k].max(), v[keys == k].min()] for k in self.g_keys], np.int64)

    def _words(self, mask):
        bits = np.zeros(256, np.uint8)
        bits[: self.N] = mask
        return np.packbits(bits, bitorder="little").view(np.uint64).copy()

    def rows(self):
        idx = self.surv
        if self.s.ordered:
            idx = idx[np.argsort(self.vals[idx], kind="stable")]
            idx = idx[:5] if self.s.order_limit else idx
        if self.limit:
            idx = idx[: self.limit]
        return idx.astype(np.uint32), [self.vals[idx].view(np.uint8).reshape(-1, 4)]

    def locate(self):
        idx = self.rows()[0]
        return (idx // 50).astype(np.uint32), (idx % 50).astype(np.uint32)

    def reserve(self, kind):
        return {"small": self.count // 3 + 1, "exact": self.count, "whole": self.N}[kind]

    def group_order_args(self, op):
        g = len(self.g_keys)
        return list(op[1]), {"all": 0, "one": 1, "half": max(1, g // 2), "more": g + 3}[op[2]]

    def perm(self, order):
        """first-seen places of the groups in the order `order` asks for"""
        g = list(range(len(self.g_keys)))
        if order is None:
            return g
        keys, limit = self.group_order_args(order)

        def part(i, kind, index, desc):
            x = int(self.g_keys[i]) if kind == GROUP_COL else int(self.g_vals[i, index])
            return -x if desc else x
        g.sort(key=lambda i: tuple(part(i, *k) for k in keys))
        return g[:limit] if limit > 0 else g

    def groups_at(self, places):
        p = np.array(places, np.int64)
        return {"keys": self.g_keys[p], "first": self.g_first[p], "counts": self.g_counts[p], "vals": self.g_vals[p],
                "key_bytes": self.g_keys[p].astype(np.uint8).reshape(-1, 1), "strings": self.g_vals[p, 1].astype(np.uint8).reshape(-1, 1)}

    def groups(self, order):
        return self.groups_at(self.perm(order))


# ---- the stand-in -----------------------------------------------------------------------------------------------------------------
FLAGS = dict(ran_select=False, ran_project=False, bitmap_valid=False, select_partial=False, bitmap_lazy=False, ran_agg=False,
             fused=False, group_order_valid=False)
MUTANTS = ("bitmap checks bitmap_valid before it settles the fused select",       # ADVICE.md, finding 1
           "a graph does not save select_partial",                                 # finding 3 (there: limit_gather_ran)
           "a run entry leaves ran_project set",
           "run_select leaves the fused-select flag set",                          # suspect 1
           "a recording stays in the live handle",                                 # suspect 2
           "count behind a stopped limit scan is the prefix's",
           "a run leaves the ordered view of the groups valid",
           "a launch takes ran_agg and the ordered view's validity from the recording",   # found by the walk on the device
           "reserve_rows behind a run loses the run's rows")                               # found by the walk on the device


class FakeGraph:
    def __init__(self, h, entries, noted):
        self.h, self.entries, self.noted, self.stale = h, entries, noted, False

    def launch(self):
        h = self.h
        if self.stale:
            raise StateError("a query recorded in this graph has moved its buffers")
        for e in self.entries:
            h._effects(e)
        live, h.R = h.R, dict(self.noted)
        if h.defect != MUTANTS[7]:
            h.R["ran_agg"] = h.R["ran_agg"] or live["ran_agg"]         # (a recorded select run neither makes nor unmakes the groups)
            h.R["group_order_valid"] = h.R["group_order_valid"] and live["group_order_valid"]
        if h.defect == MUTANTS[1]:
            h.R["select_partial"] = live["select_partial"]

    def close(self):
        pass


class FakeHandle:
    """The contract of include/imm3.h from a flag record (R) and a few "device buffers" that hold garbage until something writes them."""

    def __init__(self, s, truth, defect=None):
        self.s, self.t, self.defect = s, truth, defect
        self.R = dict(FLAGS)
        self.fused_plan = "fused" in s.name
        self.lazy_plan = "records" in s.name
        self.d_bitmap = np.full(4, GARBAGE, np.uint64)
        self.d_count, self.d_rows = GARBAGE, None
        self.epoch, self.view, self.order = 0, None, None
        self.cap = 0 if s.reserve0 is None else truth.reserve(s.reserve0)
        self.cap = max(self.cap, min(truth.limit, truth.N))   # (a query created with a limit has its row arrays from creation)
        self.capturing, self.graphs = False, []

    # the runs: what they leave in the record, and what they write
    def _select_flags(self, count_only=False):
        R = self.R
        R["ran_select"], R["bitmap_lazy"], R["select_partial"] = True, False, False
        if self.defect != MUTANTS[3]:
            R["fused"] = False
        R["bitmap_valid"] = self.s.count_stores_bitmap or not count_only

    def _select_effects(self, count_only=False):
        self.d_count = self.t.count
        if self.s.count_stores_bitmap or not count_only:
            self.d_bitmap = self.t.bitmap.copy()

    def _flags(self, entry):
        R, s = self.R, self.s
        if entry != "run":
            return self._select_flags(entry == "run_count")
        if s.kind == "agg" and self.fused_plan:
            R["fused"] = R["ran_select"] = True
        else:
            self._select_flags()
        if s.kind == "agg":
            R["ran_agg"] = True
            if self.defect != MUTANTS[6]:
                R["group_order_valid"] = False
        if s.kind == "project":
            R["ran_project"] = True
            if self.lazy_plan:
                R["bitmap_lazy"], R["bitmap_valid"] = True, False
            R["select_partial"] = self.t.stops

    def _effects(self, entry):
        s, t = self.s, self.t
        if entry != "run":
            return self._select_effects(entry == "run_count")
        if s.kind == "agg":
            self.epoch += 1                                   # (the table's slots come out in another order every time)
            if self.fused_plan:
                return
        if s.kind == "project":
            self.d_rows = t.rows()
            if self.cap == 0:
                self.cap = t.count
            if self.lazy_plan:
                self.d_count = t.count
                return
            if t.stops:
                self.d_count, self.d_bitmap = t.prefix_count, t.prefix_bitmap.copy()
                return
        self._select_effects()

    def _entry(self, entry):
        if self.capturing:
            if self.s.ordered or (self.s.kind == "project" and self.cap == 0):
                raise StateError("cannot be recorded")
        if self.defect != MUTANTS[2]:
            self.R["ran_project"] = False
        self._flags(entry)
        if not self.capturing:
            self._effects(entry)

    def run(self):
        self._entry("run")

    def run_select(self):
        self._entry("run_select")

    def run_count(self):
        self._entry("run_count")

    def sync(self):
        pass

    def ran(self, last, ran_full):
        pass

    def record(self, entries):
        saved, self.capturing = dict(self.R), True
        try:
            for e in entries:
                self._entry(e)
            g = FakeGraph(self, tuple(entries), dict(self.R))
        finally:
            self.capturing = False
            if self.defect != MUTANTS[4]:
                self.R = saved
        self.graphs.append(g)
        return g

    # the getters: settle what the last run left undone, then answer from the buffers
    def _settle(self, fused=False, lazy=False, whole=False):
        R = self.R
        if fused and R["fused"]:
            self._select_flags()
            self._select_effects()
            R["fused"] = False
        if lazy and R["bitmap_lazy"] and not R["bitmap_valid"]:
            self._select_flags()
            self._select_effects()
        if whole and R["select_partial"]:
            self._select_flags()
            self._select_effects()

    def count(self):
        if not self.R["ran_select"]:
            raise StateError("not run")
        self._settle(fused=True, whole=self.defect != MUTANTS[5])
        return self.d_count

    def device_count(self):
        self._settle(fused=True, whole=True)
        return self.d_count

    def bitmap(self):
        if not self.R["ran_select"] or (self.defect == MUTANTS[0] and not self.R["bitmap_valid"]):
            raise StateError("not run")
        self._settle(fused=True, lazy=True, whole=True)
        if not self.R["bitmap_valid"]:
            raise StateError("the last run was count-only")
        return self.d_bitmap.copy()

    def _stale(self):
        for g in self.graphs:
            g.stale = True

    def fetch_rows(self):
        if not self.R["ran_project"]:
            raise StateError("no projection has been run")
        if len(self.d_rows[0]) > self.cap:
            self.cap = len(self.d_rows[0])
            self._stale()
        return self.d_rows

    def row_count(self):
        return len(self.fetch_rows()[0])

    def locate_rows(self, idx):
        return (np.asarray(idx) // 50).astype(np.uint32), (np.asarray(idx) % 50).astype(np.uint32)

    def reserve_rows(self, n):
        if n > self.cap and self.d_rows is not None and self.defect == MUTANTS[8]:
            idx, cols = self.d_rows                            # (arrays allocated anew, nothing written to them)
            self.d_rows = (np.full_like(idx, 0xA5A5A5A5), [np.full_like(c, 0xA5) for c in cols])
        self.cap = max(self.cap, n)
        self._stale()

    def set_order(self, keys, limit):
        if self.R["ran_select"] or self.R["ran_project"] or self.R["ran_agg"]:
            raise StateError("the query has already run")

    def set_group_order(self, keys, limit):
        self.order = ("set_group_order", tuple(keys), limit) if keys else None
        self.R["group_order_valid"] = False

    def _groups(self):
        if not self.R["ran_agg"]:
            raise StateError("no aggregation has been run")
        t, g = self.t, len(self.t.g_keys)
        dense = [(p + self.epoch) % g for p in range(g)]       # where the collect put the groups this time
        if self.order is None:
            return t.groups_at(sorted(dense))
        if not self.R["group_order_valid"]:
            keys, limit = self.order[1], self.order[2]
            places = list(range(g))
            places.sort(key=lambda i: tuple((-1 if d else 1) * (int(t.g_keys[i]) if k == GROUP_COL else int(t.g_vals[i, j])) for k, j, d in keys))
            self.view = [dense.index(i) for i in (places[:limit] if limit > 0 else places)]
            self.R["group_order_valid"] = True
        return t.groups_at([dense[p] for p in self.view])

    def group_count(self):
        return len(self._groups()["first"])

    def fetch_groups(self):
        g = self._groups()
        return g["keys"], g["first"], g["counts"], g["vals"]

    def fetch_group_keys(self):
        return self._groups()["key_bytes"]

    def fetch_group_strings(self, j):
        return self._groups()["strings"]


# ---- the generator ----------------------------------------------------------------------------------------------------------------
def committed(s):
    return sequences(s, more=0)


def annotate(s, ops):
    """[(op, expectation, the kind of step before it)] under the model, a launch that may be refused taken as refused"""
    m, out, prev = Model(s), [], None
    for op in ops:
        e = m.expect(op)
        out.append((op, e, prev))
        prev = m.tag(op, e)
        m.commit(op, e.status == "ok")
    return out


@pytest.mark.parametrize("s", SUBJECTS, ids=repr)
def test_sequences_are_fixed_and_cover_every_getter_behind_every_kind_of_step(s):
    seqs = committed(s)
    assert [seed for seed, _ in seqs] == list(rsm.SEEDS) and len(seqs) == 8
    assert all(len(ops) == s.seq_len == 40 for _, ops in seqs)
    assert seqs == committed(s)                                             # a pure function of the subject and the seed
    seen = {(prev, op[0]) for _, ops in seqs for op, e, prev in annotate(s, ops) if is_getter(op)}
    missing = [(t, g) for t in s.contexts() for g in s.getters() if (t, g) not in seen]
    assert not missing, missing
    names = {op[0] for _, ops in seqs for op in ops}
    assert {"sync", "launch", "close_graph"} - names <= ({"launch", "close_graph"} if s.ordered else set())
    if s.kind == "project":
        assert {k for _, ops in seqs for op in ops if op[0] == "reserve" for k in op[1:]} == set(rsm.RESERVE_KINDS)
    if s.kind == "agg":
        orders = [op for _, ops in seqs for op in ops if op[0] == "set_group_order"]
        assert any(not op[1] for op in orders) and any(op[1] for op in orders)          # set, and removed again
        assert {op[2] for op in orders} >= {"all", "one", "half"}


@pytest.mark.parametrize("s", SUBJECTS, ids=repr)
def test_err_state_stays_the_exception(s):
    getters = errs = 0
    for seed, ops in committed(s):
        run = 0
        for op, e, _ in annotate(s, ops):
            run = run + 1 if e.status == "err" else 0
            assert run <= 6, (s, seed, op)
            if is_getter(op):
                getters += 1
                errs += e.status == "err"
    assert getters >= 50 and errs * 4 <= getters, (s, getters, errs)


def test_the_suspects_are_prefixes_of_committed_sequences():
    def starts(name, prefix):
        return any(ops[: len(prefix)] == prefix for _, ops in committed(SUBJECT_BY_NAME[name]))
    fused = "aggregation, lanes, fused select"
    assert starts(fused, [("run",), ("run_count",), ("bitmap",)])
    assert starts(fused, [("run",), ("run_select",), ("count",)])
    assert starts("select, one int32 range", [("run_count",), ("record", "run_select"), ("bitmap",)])
    assert starts("survivor records", [("run",), ("record", "run_select"), ("row_count",)])
    assert starts("one launch, unreserved", [("record", "run")])                       # refused: never run, nothing reserved
    assert starts("ordered projection", [("record", "run")])


# ---- the walker -------------------------------------------------------------------------------------------------------------------
def fails(s, defect):
    """the committed sequences of `s` on which the walker rejects the stand-in"""
    t, out = FakeTruth(s), []
    for seed, ops in committed(s):
        try:
            walk(s, seed, ops, FakeHandle(s, t, defect), t)
        except AssertionError as e:
            out.append((seed, e))
    return out


@pytest.mark.parametrize("s", SUBJECTS, ids=repr)
def test_the_walker_passes_the_honest_stand_in(s):
    bad = fails(s, None)
    assert not bad, bad[0]


@pytest.mark.parametrize("defect", MUTANTS)
def test_the_walker_fails_every_mutant(defect):
    killers = {s.name: len(f) for s in SUBJECTS for f in [fails(s, defect)] if f}
    assert killers, defect
    if defect == MUTANTS[3]:                                                # the suspects die on the very prefix that names them
        s = SUBJECT_BY_NAME["aggregation, lanes, fused select"]
        assert "step 2" in str(fails(s, defect)[0][1])
    if defect == MUTANTS[4]:
        s = SUBJECT_BY_NAME["select, one int32 range"]
        assert any(seed == 1 and "step 2" in str(e) for seed, e in fails(s, defect))


def test_a_failure_is_a_script():
    s = SUBJECT_BY_NAME["aggregation, lanes, fused select"]
    seed, e = fails(s, MUTANTS[3])[0]
    text = str(e)
    assert s.name in text and "seed %d" % seed in text and "('run',)" in text and "after [" in text
