"""GPU suite: whole statements through both engines against plain Python (stmt_fuzz_util.py; its census: test_stmt_fuzz_host.py).  The
layer above the C ABI -- the two Engines, the two SQL parsers, the host-side merge, filter and order twins -- decides which launch a
statement gets, and decides it twice.  Every seeded statement runs through the Python Engine in four configurations:

  a  blocks of 1024, one context              the table plan (or the library's refusal of a tree, and per-segment queries)
  b  blocks of 1000, one context              per-segment queries and the host merges (merge_ordered, filter_groups, order_groups)
  c  blocks of 1000, device_merge=True        per-segment queries and the device merges
  d  blocks of 1024, two contexts on device 0, device_merge=True    the segments alternate between the contexts: the _all merges

and must return what stmt_fuzz_util.expected computes over the list of row dicts; in (a) a projection must take the path
predict_path names.  The statements the grammar can spell go through host/operators.hpp's Engine as well -- tests/native/stmt_batch.cpp,
four child processes in all: both block sizes, honourAndOr off and on -- and six of them through imm3_sql itself.  The error class must
be refused by every configuration and by the batch.

IMM3_FUZZ_MORE=<n> adds n seeds behind the default set."""
import os
import shutil
import subprocess
from dataclasses import replace

import pytest

import stmt_fuzz_util as F

pytestmark = pytest.mark.gpu
MORE = int(os.environ.get("IMM3_FUZZ_MORE", "0") or 0)      # extra seeds for a long hunt (default: the bounded set)
SEEDS = list(range(F.SEEDS + MORE))
HERE = os.path.dirname(os.path.abspath(__file__))
CLI_FLAGS = ("--order-by", "--string-ranges", "--having")


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    rows, dirs, _ = F.make_tables(tmp_path_factory.mktemp("stmt_fuzz"))
    return rows, dirs, F.Data(rows)


@pytest.fixture(scope="module")
def managers(tables):
    """{configuration: (GpuSegmentManager, device_merge, block size, contexts)}, staged once"""
    from immutable3_amd import native
    from immutable3_amd.operators import GpuSegmentManager
    from immutable3_amd.storage import SegmentManager
    _, dirs, _ = tables
    ctxs = [native.Context(0) for _ in range(2)]
    one, ragged, two = GpuSegmentManager(SegmentManager(dirs[1024])), GpuSegmentManager(SegmentManager(dirs[1000])), GpuSegmentManager(SegmentManager(dirs[1024]), ctxs)
    assert one.device_table(F.TABLE) is not None and ragged.device_table(F.TABLE) is None and two.device_table(F.TABLE) is None
    assert one.getTableSegmentCount(F.TABLE) == ragged.getTableSegmentCount(F.TABLE) == 3
    yield {"a": (one, False, 1024, 1), "b": (ragged, False, 1000, 1), "c": (ragged, True, 1000, 1), "d": (two, True, 1024, 2)}
    for m in (one, ragged, two):
        m.close()
    for c in ctxs:
        c.close()


def refused(run):
    """run() must REFUSE: the ADT's constructors (ValueError), the operators (a plain Exception: "Unknown Aggregate type", "Unsupported
    condition") or the library at creation (Imm3Error, but no device error).  A TypeError or the like is a crash, not a refusal."""
    from immutable3_amd import native
    with pytest.raises(Exception) as e:
        run()
    assert type(e.value) in (Exception, ValueError, native.Imm3Error), repr(e.value)
    assert not isinstance(e.value, native.Imm3Error) or e.value.code in (native.ERR_ARG, native.ERR_UNSUPPORTED_CONDITION), repr(e.value)


def run_python(engine, s):
    """the statement through one Engine, in the reference's terms: a projection's value tuples; an aggregation's [(key, {alias: value})]
    and its Row(...) texts (every aggregator's get() and repr())"""
    q = F.to_query(s)
    if s.kind == "project":
        return [tuple(r) for r in engine.execute(q)], None
    got = engine.execute_agg(q)
    plain = [(k, {alias: a.get() for alias, a in m.items()}) for k, m in got.items()]       # (a float get() equals its integer only when it is integral)
    return plain, ["Row(" + ",".join(a.repr() for a in m.values()) + ")" for m in got.values()]


@pytest.mark.parametrize("seed", SEEDS)
def test_python_engine_in_four_configurations(tables, managers, seed):
    from immutable3_amd.operators import Engine
    rows, _, data = tables
    for i, s in enumerate(F.statements(seed, data)):
        if s.error is not None:
            with pytest.raises(F.Refused):
                F.expected(rows, s)
            for name, (gsm, device_merge, _, _) in managers.items():
                engine = Engine(gsm, honour_and_or=s.honour_and_or, device_merge=device_merge, honour_not_match=s.honour_not_match)
                refused(lambda: run_python(engine, s))
            continue
        want = F.expected(rows, s)
        text = None if s.kind == "project" else F.rows_text(s, want)
        for name, (gsm, device_merge, block, contexts) in managers.items():
            engine = Engine(gsm, honour_and_or=s.honour_and_or, device_merge=device_merge, honour_not_match=s.honour_not_match)
            got, got_text = run_python(engine, s)                       # (an Imm3Error here fails the test: nothing is caught)
            assert got == want and got_text == text, (seed, i, name, s)
            path = F.predict_path(s, block, contexts)
            if s.kind == "project" and path != "either":
                assert (engine.execute_table_columns(F.to_query(s)) is not None) == (path == "table"), (seed, i, name, path, s)


# ---- the C++ engine ------------------------------------------------------------------------------------------------------------------
def sections(stdout):
    """{line no: (header text behind the number, [Row lines])} of a stmt_batch run"""
    out, cur = {}, None
    for line in stdout.splitlines():
        if line.startswith("== "):
            n, _, head = line[3:].partition(" ")
            cur = out[int(n)] = (head, [])
        else:
            assert cur is not None and line.startswith("Row("), line
            cur[1].append(line)
    return out


def pick_six(cases, got):
    """six spellable statements that between them hold every clause, with more than one row to print where there is such a statement;
    got: a batch's sections"""
    wants = [lambda s: s.kind == "project" and s.order_by and s.limit > 0, lambda s: s.kind == "project" and F.has_or(s.where),
             lambda s: s.kind == "agg" and s.having is not None and s.having[0] in ("and", "or"), lambda s: s.kind == "agg" and s.order_by and s.limit > 0 and s.group,
             lambda s: any(l[2] in F.RANGE_OPS for l in F.leaves_of(s.where)), lambda s: s.kind == "agg" and s.where is not None and "order_no" in F.used_columns(s)]
    out = []
    for w in wants:
        fit = [k for k, (s, _) in enumerate(cases) if s.error is None and w(s) and k not in out]
        out.append(next((k for k in fit if len(got[k + 1][1]) > 1), fit[0]))
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cpp_engine_in_four_batches(tables, tmp_path):
    rows, dirs, data = tables
    root = os.path.dirname(HERE)
    exe, lib = str(tmp_path / "stmt_batch"), os.path.join(root, "immutable3_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O0", os.path.join(HERE, "native", "stmt_batch.cpp"), "-o", exe, "-L", lib, "-limm3", f"-Wl,-rpath,{lib}"])
    cases = [(s, F.render(s)) for seed in SEEDS for s in F.statements(seed, data) if F.render(s) is not None]
    assert len(cases) >= 60
    results = {}
    for hao in (False, True):
        wanted = []                                                     # per statement: its Row lines, or None where both engines must refuse
        for (s, _) in cases:
            try:
                v = replace(s, honour_and_or=hao, honour_not_match=False)
                wanted.append(F.rows_text(v, F.expected(rows, v)))
            except F.Refused:
                wanted.append(None)
        assert sum(w is None for w in wanted) >= 4
        listing = tmp_path / f"statements{int(hao)}.sql"
        listing.write_text(encoding="utf-8", data="".join(("!" if w is None else "") + sql + "\n" for (_, sql), w in zip(cases, wanted)))
        for block in F.BLOCKS:
            p = subprocess.run([exe, dirs[block], str(int(hao)), str(listing)], capture_output=True, text=True, encoding="utf-8", timeout=300)
            assert p.returncode == 0, (block, hao, p.returncode, p.stdout[-1500:], p.stderr[-1500:])    # (no later child after a failure)
            got = sections(p.stdout)
            assert sorted(got) == list(range(1, len(cases) + 1))
            for k, ((s, sql), want) in enumerate(zip(cases, wanted)):
                head, lines = got[k + 1]
                what = (block, hao, sql)
                if want is None:
                    assert head.startswith("error: ") and not lines, what
                    continue
                assert head.startswith("path: ") and lines == want, what
                path = F.predict_path(replace(s, honour_and_or=hao, honour_not_match=False), block)
                if path != "either":
                    assert head.startswith("path: one table query" if path == "table" else "path: per-segment queries"), (what, head)
            results[(block, hao)] = got
    # imm3_sql itself, with its switches, prints what the batch printed: six statements, the block sizes in turn
    for n, k in enumerate(pick_six(cases, results[(1024, False)])):
        _, sql = cases[k]
        hao = results[(1024, True)][k + 1][0].startswith("path: ")       # (honoured where the statement runs that way)
        block = F.BLOCKS[n % 2]
        head, lines = results[(block, hao)][k + 1]
        p = subprocess.run([os.path.join(F.BIN, "imm3_sql"), *CLI_FLAGS, *(("--honour-and-or",) if hao else ()), "--explain", "-q", sql, "-d", dirs[block]],
                           capture_output=True, text=True, encoding="utf-8", timeout=120)
        assert p.returncode == 0, (sql, p.stdout[-1500:], p.stderr[-1500:])
        assert p.stdout.splitlines() == lines and head in p.stderr, (sql, block, head, p.stderr)
