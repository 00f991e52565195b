"""Random call sequences on ONE query handle, and the model that says what every call must answer.

What a getter does is decided by the run record of the handle (csrc/imm3_handles.h: QueryRunState): three run entries set it, a graph
replay restores it whole, the lazy settle steps of the getters clear it.  The suites elsewhere vary data, plans and shapes and keep
the ORDER OF CALLS fixed; this file varies the order.  Three pieces, none of which needs a device:

  Model      include/imm3.h restated as "is this getter defined now": the data are immutable, so the VALUE of a getter is a pure
             function of the query (and, for groups, of the group order last set) -- the model tracks only which run entry executed
             last, whether a full run ever executed, the graphs recorded so far and the order set on the groups.
  SUBJECTS   one query per plan the library has, at the smallest shape that still takes that plan; tests/test_gpu_run_state.py builds
             them on the device, tests/test_run_state_host.py drives a stand-in.
  sequences  seeded operation lists per subject, drawn so that every getter follows every kind of run, replay, recording and
             reservation (test_run_state_host.py asserts that coverage).

walk() runs one sequence against any object with the handle's methods and holds every answer to the model.

Where the header is silent the model decides (and the header now says so):
  - between imm3_ctx_capture_end and the first launch a handle describes the last run that EXECUTED, not the recorded one;
  - a recording that is refused (an ordered query, row arrays that do not exist yet) leaves the handle as it was;
  - imm3_query_reserve_rows behind a run leaves that run's rows readable;
  - a projecting query is recorded (imm3_query_run and imm3_query_run_select alike) only once its row arrays exist: after an
    executed imm3_query_run or a reservation, or from creation when it has a limit (the header's "must have run once before").
"""
import os
import random
from collections import namedtuple

ERR_STATE = 7
RUN_ENTRIES = ("run", "run_select", "run_count")
SELECT_GETTERS = ("count", "bitmap", "device_count")
ROW_GETTERS = ("row_count", "fetch_rows")
GROUP_GETTERS = ("group_count", "fetch_groups", "fetch_group_keys")
RESERVE_KINDS = ("small", "exact", "whole")      # below the survivors / exactly the survivors / every row of the segment
SEEDS = tuple(range(8))
SEQ_LEN = 40


class StateError(Exception):
    """what the stand-in raises where the library answers IMM3_ERR_STATE (native.Imm3Error carries the same `code`)"""
    code = ERR_STATE


class Subject:
    """One query under test, as far as the model needs to know it.
    kind: "select" (no SELECT list), "project", "agg".  count_stores_bitmap: does imm3_query_run_count store the bitmap -- not when the
    select chain is one fused launch over a segment, nor for a tile-form tree over a segment (include/imm3.h).  limit: "" none,
    "small" below the survivors, "large" above them.  reserve0: a reservation made before the first run.  tuning: the variant and grid
    the sequence runs under.  order_keys: the (kind, index) pairs imm3_query_set_group_order may be given.  string_agg: the index of
    a string MAX aggregate, or None."""

    def __init__(self, name, kind, count_stores_bitmap, table=False, limit="", ordered=False, order_limit=False, reserve0=None,
                 tuning=(0, 0), order_keys=(), string_agg=None, seq_len=SEQ_LEN):
        self.name, self.kind, self.count_stores_bitmap, self.table = name, kind, count_stores_bitmap, table
        self.limit, self.ordered, self.order_limit, self.reserve0, self.tuning = limit, ordered, order_limit, reserve0, tuning
        self.order_keys, self.string_agg, self.seq_len = tuple(order_keys), string_agg, seq_len

    def getters(self):
        g = list(SELECT_GETTERS)
        if self.kind == "project":
            g += list(ROW_GETTERS) + (["locate_rows"] if self.table else [])
        if self.kind == "agg":
            g += list(GROUP_GETTERS) + (["fetch_group_strings"] if self.string_agg is not None else [])
        return tuple(g)

    def contexts(self):
        """the kinds of step every getter has to be seen directly behind"""
        tags = list(RUN_ENTRIES)
        tags += ["refused"] if self.ordered else ["launch:run", "launch:run_select", "capture_end"]
        if self.kind == "project":
            tags.append("reserve")
        return tuple(tags + ["getter"])

    def __repr__(self):
        return self.name


GROUP_COL, AGG = 0, 1   # imm3_query_set_group_order's key kinds
NARROW_KEYS = ((GROUP_COL, 0), (AGG, 0), (AGG, 1))
SUBJECTS = (
    Subject("select, one int32 range", "select", False),
    Subject("select, PFOR_INT and two 2-byte strings", "select", True),
    Subject("one launch, unreserved", "project", False, tuning=(12, 0)),
    Subject("one launch, reservation too small", "project", False, tuning=(12, 0), reserve0="small"),
    Subject("one launch, exact reservation", "project", False, tuning=(12, 0), reserve0="exact"),
    Subject("survivor records", "project", False, tuning=(12, 0)),
    Subject("bitmap path", "project", False, tuning=(3, 0)),
    Subject("segment limit, small", "project", False, limit="small"),
    Subject("segment limit, small, two launches", "project", False, limit="small", tuning=(15, 0)),
    Subject("segment limit above the count", "project", False, limit="large"),
    Subject("table limit", "project", True, table=True, limit="small", tuning=(0, 4)),
    Subject("aggregation, lanes, fused select", "agg", False, order_keys=NARROW_KEYS),
    Subject("aggregation, lanes, select launch", "agg", False, tuning=(17, 0), order_keys=NARROW_KEYS),
    Subject("aggregation, 64 keys", "agg", False, order_keys=NARROW_KEYS),
    Subject("aggregation, 16-byte key and string MAX", "agg", False, order_keys=((AGG, 0), (AGG, 2)), string_agg=1),
    Subject("tile tree with OR and NOT", "select", False),
    Subject("generic tree", "project", True, tuning=(1, 0)),
    Subject("table tile tree, limit", "project", True, table=True, limit="small"),
    Subject("ordered projection", "project", False, ordered=True, tuning=(12, 0)),
    Subject("ordered projection, limit", "project", False, ordered=True, order_limit=True, tuning=(12, 0)),
    Subject("table projection, four segments", "project", True, table=True, tuning=(12, 0)),
    Subject("table aggregation, four segments", "agg", True, table=True, order_keys=NARROW_KEYS),
)
SUBJECT_BY_NAME = {s.name: s for s in SUBJECTS}

Exp = namedtuple("Exp", "status value")   # status: "ok" / "err" (IMM3_ERR_STATE) / "either"; value: what an ok answer is compared with


def is_getter(op):
    return op[0] in SELECT_GETTERS or op[0] in ROW_GETTERS or op[0] in GROUP_GETTERS or op[0] in ("locate_rows", "fetch_group_strings")


class Model:
    def __init__(self, subject):
        self.s = subject
        self.last = None           # the run entry that executed last, directly or through a launch
        self.ran_full = False      # an imm3_query_run has executed
        self.group_order = None    # the set_group_order operation in force
        self.graphs = {}           # id -> [entries, firm]; firm: the launch must succeed
        self.n_recorded = 0
        # the row arrays: 0 none yet, 1 too small for the survivors, 2 large enough
        self.cap = {None: 0, "small": 1, "exact": 2, "whole": 2}[subject.reserve0]
        if subject.kind == "project" and subject.limit:
            self.cap = 2                                                # (a query created with a limit has its arrays from creation)

    def expect(self, op):
        s, name = self.s, op[0]
        if name in RUN_ENTRIES or name in ("sync", "close_graph", "reserve", "set_group_order"):
            return Exp("ok", None)
        if name == "set_order":                                        # (only ever drawn behind a run)
            return Exp("err", None)
        if name == "record":
            if s.ordered or (s.kind == "project" and self.cap == 0):
                return Exp("err", None)
            assert self.last is not None, "a sequence records only queries that have run once (include/imm3.h)"
            return Exp("ok", None)
        if name == "launch":
            return Exp("ok" if self.graphs[op[1]][1] else "either", None)
        if name in ("count", "device_count"):
            assert name == "count" or self.last is not None, "the device word is read only behind a run"
            return Exp("ok", "count") if self.last is not None else Exp("err", None)
        if name == "bitmap":
            if self.last is None or (self.last == "run_count" and not s.count_stores_bitmap):
                return Exp("err", None)
            return Exp("ok", "bitmap")
        if name in ROW_GETTERS or name == "locate_rows":
            return Exp("ok", name) if (s.kind == "project" and self.last == "run") else Exp("err", None)
        if name in GROUP_GETTERS or name == "fetch_group_strings":
            return Exp("ok", name) if (s.kind == "agg" and self.ran_full) else Exp("err", None)
        raise AssertionError("unknown operation %r" % (op,))

    def commit(self, op, ok):
        """the operation answered ok / IMM3_ERR_STATE"""
        name = op[0]
        if name in RUN_ENTRIES:
            self.last = name
            if name == "run":
                self.ran_full = True
                if self.cap == 0:
                    self.cap = 2                                        # (an unreserved first run sizes the arrays from the count)
        elif name == "record" and ok:
            self.graphs[self.n_recorded] = [tuple(op[1:]), self.cap != 1]   # (arrays that will be outgrown: the graph may go stale)
            self.n_recorded += 1
        elif name == "launch":
            entries = self.graphs[op[1]][0]
            if ok:
                self.last = entries[-1]
                self.ran_full = self.ran_full or "run" in entries
            else:
                del self.graphs[op[1]]                                  # (stale: the walker drops it)
        elif name == "close_graph":
            del self.graphs[op[1]]
        elif name == "reserve":
            for g in self.graphs.values():
                g[1] = False
            self.cap = max(self.cap, 1 if op[1] == "small" else 2)
        elif name == "set_group_order":
            self.group_order = op if op[1] else None
        elif (name in ROW_GETTERS or name == "locate_rows") and ok and self.cap == 1:
            for g in self.graphs.values():                              # (the arrays grew under the getter)
                g[1] = False
            self.cap = 2

    def tag(self, op, exp):
        """the kind of step `op` is for the getter behind it (Subject.contexts), None when it is none of them"""
        name = op[0]
        if name in RUN_ENTRIES:
            return name
        if name == "record":
            return "capture_end" if exp.status == "ok" else "refused"
        if name == "launch":
            return "launch:" + self.graphs[op[1]][0][-1] if exp.status == "ok" else None
        if name == "reserve":
            return "reserve"
        if is_getter(op) and exp.status == "ok":
            return "getter"
        return None


# ---- sequences -----------------------------------------------------------------------------------------------------------------
ERR_SHARE = 0.23         # the generator's own bound on getter steps that expect IMM3_ERR_STATE (the host test asserts a quarter)
ERR_RUN = 5              # ... and on such steps in a row (asserted: six)


def openings(s):
    """how the sequences of the first seeds begin: the call orders read out of the code as suspects"""
    rec = ("record", "run_select")
    out = {0: [("run",), ("run_count",), ("bitmap",)],                   # a fused select's flag behind a count-only run
           1: [("run_count",), rec, ("bitmap",)],                         # a recording behind a run that stored no bitmap
           2: [("run",), rec, ("row_count",)] if s.kind == "project" else [("run",), ("run_select",), ("count",)],
           3: [("run",), ("run_select",), ("count",), ("bitmap",)]}
    if (s.kind == "project" and Model(s).cap == 0) or s.ordered:
        out[4] = [("record", "run"), ("count",)]                         # refused: nothing has run, no rows are reserved
    return out


class _Gen:
    def __init__(self, s):
        self.s = s
        self.need = {(t, g) for t in s.contexts() for g in s.getters()}
        self.n_getters = self.n_errs = 0

    def allowed(self, m, op, err_run):
        e = m.expect(op)
        if e.status != "err":
            return True
        return err_run < ERR_RUN and (not is_getter(op) or self.n_errs + 1 <= ERR_SHARE * (self.n_getters + 1))

    def record_op(self, rng, m, last_entry=None):
        s = self.s
        if s.ordered:
            return ("record", "run")
        if m.last is None:
            return ("run",)
        if last_entry is None:
            last_entry = rng.choice(("run", "run_select"))
        if s.kind == "project" and m.cap == 0:
            return ("run",)
        first = rng.choice((None, None, "run", "run_select"))
        return ("record", first, last_entry) if first else ("record", last_entry)

    def realise(self, rng, m, tag):
        """an operation that makes the next step one of kind `tag`"""
        if tag in RUN_ENTRIES:
            return (tag,)
        if tag in ("capture_end", "refused"):
            return self.record_op(rng, m)
        if tag.startswith("launch:"):
            have = [k for k, (entries, firm) in sorted(m.graphs.items()) if firm and entries[-1] == tag[7:]]
            return ("launch", rng.choice(have)) if have else self.record_op(rng, m, tag[7:])
        if tag == "reserve":
            return ("reserve", rng.choice(RESERVE_KINDS))
        fine = [g for g in self.s.getters() if (g != "device_count" or m.last is not None) and m.expect((g,)).status == "ok"]
        return (rng.choice(fine),) if fine else ("run",)

    def group_order_op(self, rng):
        keys = list(self.s.order_keys)
        rng.shuffle(keys)
        keys = keys[: rng.randint(0, len(keys))]                          # (no key: the order is removed)
        return ("set_group_order", tuple((k, i, rng.randint(0, 1)) for k, i in keys), rng.choice(("all", "one", "half", "more")))

    def random_op(self, rng, m):
        s = self.s
        r = rng.random()
        if r < 0.26:
            return (rng.choice(RUN_ENTRIES),)
        if r < 0.33:
            return self.record_op(rng, m)
        if r < 0.45 and m.graphs:
            return ("launch", rng.choice(sorted(m.graphs)))
        if r < 0.51 and m.graphs:
            return ("close_graph", rng.choice(sorted(m.graphs)))
        if r < 0.55 and s.kind == "project":
            return ("reserve", rng.choice(RESERVE_KINDS))
        if r < 0.68 and s.kind == "agg":
            return self.group_order_op(rng)
        if r < 0.73:
            return ("sync",)
        if r < 0.75 and s.kind == "project" and not s.limit and m.last is not None:
            return ("set_order",)
        g = rng.choice(s.getters())
        return (g,) if (g != "device_count" or m.last is not None) else ("run_count",)

    def choose(self, rng, m, prev_tag, prev_op, err_run):
        for _ in range(64):
            op = None
            if prev_tag:                                                 # a getter that has not been seen behind this kind of step
                cand = [g for g in self.s.getters() if (prev_tag, g) in self.need and (g,) != prev_op
                        and (g != "device_count" or m.last is not None) and self.allowed(m, (g,), err_run)]
                scarce = [g for g in cand if m.expect((g,)).status == "err"]   # (pairs that can only be seen while the budget allows)
                if cand and rng.random() < 0.95:
                    op = (rng.choice(scarce or cand),)
            tight = self.n_errs + 1 > ERR_SHARE * (self.n_getters + 1)   # no refusal can be afforded: answered getters first
            if op is None and tight and rng.random() < 0.6:
                op = self.realise(rng, m, "getter")
            if op is None and self.need and not tight and rng.random() < 0.75:         # ... or a step of a kind that still lacks getters
                op = self.realise(rng, m, rng.choice(sorted(self.need))[0])
            if op is None:
                op = self.random_op(rng, m)
                if self.need and is_getter(op) and m.expect(op).status == "err":
                    continue                                              # (the budget of refusals goes to the pairs still missing first)
            if op[0] == "launch" and not m.graphs[op[1]][1]:
                return op, ("run",)                                       # (a launch that may be refused: a run entry behind it settles the state)
            if self.allowed(m, op, err_run):
                return op, None
        return ("run",), None

    def sequence(self, seed):
        s = self.s
        rng = random.Random("%s/%d" % (s.name, seed))
        m = Model(s)
        ops, queue = [], list(openings(s).get(seed, []))
        prev_tag, prev_op, err_run = None, None, 0
        while len(ops) < s.seq_len:
            if queue:
                op = queue.pop(0)
            else:
                op, then = self.choose(rng, m, prev_tag, prev_op, err_run)
                if then:
                    queue.append(then)
            e = m.expect(op)
            tag = m.tag(op, e)
            if is_getter(op):
                self.n_getters += 1
                self.n_errs += e.status == "err"
                self.need.discard((prev_tag, op[0]))
            err_run = err_run + 1 if e.status == "err" else 0
            m.commit(op, e.status == "ok")                                # (a launch that may be refused counts as refused: a run entry follows)
            ops.append(op)
            prev_tag, prev_op = tag, op
        return ops


def sequences(subject, more=None):
    """[(seed, operations)] of a subject: the committed seeds, and IMM3_FUZZ_MORE further ones"""
    if more is None:
        more = int(os.environ.get("IMM3_FUZZ_MORE", "0") or 0)
    gen = _Gen(subject)
    return [(seed, gen.sequence(seed)) for seed in list(SEEDS) + [len(SEEDS) + k for k in range(more)]]


# ---- the walker -----------------------------------------------------------------------------------------------------------------
def _same(a, b):
    import numpy as np
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_value(value, got, truth, order, where):
    if value == "count":
        assert int(got) == int(truth.count), (where, int(got), int(truth.count))
    elif value == "bitmap":
        assert _same(got, truth.bitmap), (where, "bitmap words differ")
    elif value == "row_count":
        assert int(got) == len(truth.rows()[0]), (where, int(got), len(truth.rows()[0]))
    elif value in ("fetch_rows", "locate_rows"):
        idx, cols = got[0]
        want_idx, want_cols = truth.rows()
        assert _same(idx, want_idx), (where, "row indices differ")
        assert len(cols) == len(want_cols) and all(_same(c, w) for c, w in zip(cols, want_cols)), (where, "a SELECT-list column differs")
        if value == "locate_rows":
            seg, row = got[1]
            want_seg, want_row = truth.locate()
            assert _same(seg, want_seg) and _same(row, want_row), (where, "(segment, row) differ")
    else:
        g = truth.groups(order)
        if value == "group_count":
            assert int(got) == len(g["first"]), (where, int(got), len(g["first"]))
        elif value == "fetch_groups":
            for have, name in zip(got, ("keys", "first", "counts", "vals")):
                assert _same(have, g[name]), (where, name, "differ")
        elif value == "fetch_group_keys":
            assert _same(got, g["key_bytes"]), (where, "group key bytes differ")
        else:
            assert _same(got, g["strings"]), (where, "string maxima differ")


def walk(subject, seed, ops, handle, truth):
    """Run `ops` on `handle` (a DeviceQuery behind test_gpu_run_state.Handle, or the stand-in) and hold every answer to the model:
    IMM3_ERR_STATE exactly where the model says so, and every value equal to `truth`'s."""
    m = Model(subject)
    graphs, done = {}, []
    try:
        for step, op in enumerate(ops):
            where = "%s, seed %d, step %d: %r after %r" % (subject.name, seed, step, op, done)
            exp = m.expect(op)
            name, got, ok = op[0], None, True
            try:
                if name == "record":
                    graphs[m.n_recorded] = handle.record(op[1:])
                elif name == "launch":
                    graphs[op[1]].launch()
                elif name == "close_graph":
                    graphs.pop(op[1]).close()
                elif name == "reserve":
                    handle.reserve_rows(truth.reserve(op[1]))
                elif name == "set_group_order":
                    handle.set_group_order(*truth.group_order_args(op))
                elif name == "set_order":
                    handle.set_order([(0, False)], 0)
                elif name == "fetch_group_strings":
                    got = handle.fetch_group_strings(subject.string_agg)
                elif name == "locate_rows":
                    rows = handle.fetch_rows()
                    got = (rows, handle.locate_rows(rows[0]))
                elif name == "fetch_rows":
                    got = (handle.fetch_rows(),)
                else:
                    got = getattr(handle, name)()
            except Exception as e:                                       # noqa: BLE001 -- only IMM3_ERR_STATE is an answer
                if getattr(e, "code", None) != ERR_STATE:
                    raise AssertionError("%s: %r" % (where, e)) from e
                ok = False
            assert ok or exp.status != "ok", (where, "IMM3_ERR_STATE where the model defines the answer")
            assert not ok or exp.status != "err", (where, "an answer where the model says IMM3_ERR_STATE")
            if ok and exp.value:
                _check_value(exp.value, got, truth, m.group_order, where)
            if name == "launch" and not ok:
                graphs.pop(op[1]).close()
            m.commit(op, ok)
            if ok and (name in RUN_ENTRIES or name == "launch"):
                handle.ran(m.last, m.ran_full)                             # (the subject checks that it still takes the plan it names)
            done.append(op)
    finally:
        for g in graphs.values():
            g.close()
