"""What the one-column-pass matrix shares (test_gpu_column_pass_matrix.py, test_column_pass_host.py): the layouts, the tile-to-wave
walk restated, the columns and the predicates of every cell, and the references -- numpy and Python `bytes` only.

The three kernels (k_filter_str_rows, k_filter_str_range, k_filter_int_list; csrc/imm3_pass.h is what they share) are one wave per
1024-row tile, `first = block * 4 + wave`, `step = grid * 4`.  The layouts here are ten tiles of one segment and fourteen of a table, so
that under one work-group a wave walks three or four tiles, full and partial ones in every order.

Rows come from str_rows_util.pool_for (the wanted values t0 and t1, rows that differ from t0 in one byte of each dword) and
str_range_util.neighbours (rows around a bound); the range bounds ARE t0 and t1 in byte order, so one column serves Match and the
range, and one pinned row (the lower bound) is selected by every list and every range."""
import functools

import numpy as np

import str_range_util as R
from int_in_util import isin
from str_rows_util import pool_for

TILE = 1024
WAVES = 4                                       # waves per work-group (kWavesPerBlock)
K_MAX_MATCH = 8                                 # csrc/imm3_internal.h: kMaxMatch (test_column_pass_host.py holds it against the library)
WIDTHS = [4, 8, 12, 16, 20, 24, 28, 32, 40, 256]
GRIDS = [0, 1, 3]                               # set_tuning's grid_blocks: the default, four waves own everything, a step of 12
LAST_ROWS = [1, 63, 64, 65, 1023]               # the rows of a segment's tenth tile
# name -> rows per segment.  The table: tiles F P1 | P1 | F P700 | | F P63 | F F P1023 | F P65 | P64 | F
LAYOUTS = {f"segment-{r}": [9 * TILE + r] for r in LAST_ROWS}
LAYOUTS["table"] = [1025, 1, 1024 + 700, 0, 1024 + 63, 2048 + 1023, 1024 + 65, 64, 1024]
EMPTIED_TILE = 3                                # the tile (full in every layout) where the `gate` column keeps no row
FORMS = ["I8", "ARGS", "LDS", "GLOBAL"]         # k_filter_int_list's, in native.INT_LIST_* order


def blocks_of(n):
    return [TILE] * (n // TILE) + ([n % TILE] if n % TILE else [])


def instance_of(width):
    """<P, C, TAIL> of the string kernels at this width: IMM3_STR_LAUNCH_BY_WIDTH (csrc/imm3_strmatch.hip), restated"""
    if width <= 16:
        return {4: (1, 1, False), 8: (2, 2, False), 12: (3, 1, False), 16: (4, 4, False)}[width]
    return (4, 4 if width % 16 == 0 else 2 if width % 8 == 0 else 1, True)


def tiles_of(layout):
    """[(segment, first row in the segment, valid rows)] in tile-table order"""
    return [(si, t * TILE, min(TILE, n - t * TILE)) for si, n in enumerate(LAYOUTS[layout]) for t in range((n + TILE - 1) // TILE)]


def default_grid(n_tiles):
    return max(1, (n_tiles + WAVES - 1) // WAVES)  # (the caps, 512 and 1024 work-groups, are far away)


def walks(n_tiles, grid):
    """per wave of the launch, the tiles it walks: first = block * 4 + wave, step = grid * 4"""
    g = grid if grid > 0 else default_grid(n_tiles)
    return [list(range(first, n_tiles, g * WAVES)) for first in range(g * WAVES)]


# ---- the rows of a tile ----------------------------------------------------------------------------------------------------------
# survivors of both passes; a row the string / list pass selects and the int8 pass before it drops; a row only the int8 pass keeps
PIN_SELECTED = [0, 63, 64, 511, 512]            # ... and the tile's last valid row
PIN_SELECTED_DROPPED, PIN_OUT_KEPT, PIN_OUT_DROPPED = 1, 2, 3
PIN_ZERO, PIN_ZERO_DROPPED = 200, 201           # full tiles only


def pins(n_valid):
    """position -> what is pinned there ("sel", "sel_dropped", "out", "out_dropped", "zero", "zero_dropped") in a tile of n_valid rows"""
    p = {}
    if n_valid == TILE:
        p[PIN_ZERO], p[PIN_ZERO_DROPPED] = "zero", "zero_dropped"
    if n_valid > PIN_OUT_DROPPED + 1:
        p[PIN_SELECTED_DROPPED], p[PIN_OUT_KEPT], p[PIN_OUT_DROPPED] = "sel_dropped", "out", "out_dropped"
    for r in PIN_SELECTED + [n_valid - 1]:
        if r < n_valid:
            p[r] = "sel"
    return p


def int8_columns(rng, layout):
    """per segment (age, gate): age > 0 keeps about half the rows of every tile; gate is age except in EMPTIED_TILE, where it keeps none"""
    out = [[np.zeros(n, np.int8), None] for n in LAYOUTS[layout]]
    for ti, (si, r0, nv) in enumerate(tiles_of(layout)):
        a = rng.choice(np.array([-100, -7, -1, 1, 9, 127], np.int8), size=nv)
        for r, what in pins(nv).items():
            a[r] = -5 if what.endswith("dropped") else 5
        out[si][0][r0:r0 + nv] = a
    for s in out:
        s[1] = s[0].copy()
    si, r0, nv = tiles_of(layout)[EMPTIED_TILE]
    assert nv == TILE
    out[si][1][r0:r0 + nv] = -5
    return [tuple(s) for s in out]


def dword_steps(bound, width):
    """rows that equal `bound` up to dword d and differ from it in one byte there, for every dword d, on either side of the bound;
    those behind the 16-byte prefix share it and leave the tail loop at every depth"""
    rows = []
    for d in range(width // 4):
        at = 4 * d + d % 4
        for delta in (1, -1):
            rows.append(bound[:at] + bytes([(bound[at] + delta) & 0xFF]) + bound[at + 1:])
    return rows


class StringCase:
    """One string column of one width over one layout, with what is asked of it.  rows[s]: uint8[n, width] per segment; age / gate:
    int8 per segment; lists: [(values, what)] for Match; ranges: [(lo, hi, what)]"""

    def __init__(self, width, layout):
        self.width, self.layout, self._masks = width, layout, {}
        rng = np.random.default_rng(7000 + 31 * width + len(layout) + sum(LAYOUTS[layout]))
        pool, t0, t1 = pool_for(rng, width)
        self.lo, self.hi = sorted((bytes(t0), bytes(t1)))
        assert self.lo < self.hi
        k = 16 if width > 16 else width - 1                # lo and hi2 share their first 16 bytes (up to 16 bytes wide: all but the last)
        self.hi2 = self.lo[:k] + bytes([self.lo[k] + 0x30]) + self.lo[k + 1:]
        self.zero, self.out = b"\x00" * width, b"\xff" * width
        rows = [bytes(p) for p in pool]
        for b in (self.lo, self.hi, self.hi2):
            rows += R.neighbours(b, width) + dword_steps(b, width)
        rows = sorted(set(rows) - {self.zero, self.out})
        self.pool = R.rows_array(rows, width)
        assert self.pool.shape[0] < TILE - 16              # a full tile holds every row of the pool beside its pinned rows
        pinned = {"sel": self.lo, "sel_dropped": self.lo, "out": self.out, "out_dropped": self.out, "zero": self.zero, "zero_dropped": self.zero}
        self.rows = [np.zeros((n, width), np.uint8) for n in LAYOUTS[layout]]
        for si, r0, nv in tiles_of(layout):
            t = self.pool[rng.integers(0, self.pool.shape[0], size=nv)].reshape(nv, width).copy()
            p = pins(nv)
            free = np.array([r for r in range(nv) if r not in p], dtype=np.int64)
            if free.size >= self.pool.shape[0]:
                t[rng.permutation(free)[: self.pool.shape[0]]] = self.pool
            for r, what in p.items():
                t[r] = np.frombuffer(pinned[what], np.uint8)
            self.rows[si][r0:r0 + nv] = t
        self.age, self.gate = zip(*int8_columns(rng, layout))
        absent = [bytes(rng.integers(65, 91, size=width).astype(np.uint8)) for _ in range(K_MAX_MATCH + 2)]   # upper case: in no row
        near = self.lo[:-1] + bytes([self.lo[-1] ^ 0x40])
        short, long_ = [self.lo, self.hi, near], [self.hi, self.lo[:-1], self.lo + b"x"] + absent + [self.lo]
        assert len(set(short)) <= K_MAX_MATCH - 1 and len({v for v in long_ if len(v) == width}) > K_MAX_MATCH
        self.lists = [(short, "short"), (short + [self.zero], "short, zero"), (long_, "long"), ([self.zero] + long_, "long, zero")]
        self.ranges = [(self.lo, self.hi, "full width"), (b"", self.hi, "up to hi"), (self.lo, self.hi2, "bounds share their prefix"),
                       (self.lo, self.lo, "lo == hi")]

    def match_masks(self, values):
        """per segment bool[n] (computed once per list)"""
        key = ("match", tuple(values))
        if key not in self._masks:
            self._masks[key] = [match_mask(r, values) for r in self.rows]
        return self._masks[key]

    def range_masks(self, lo, hi):
        key = ("range", lo, hi)
        if key not in self._masks:
            self._masks[key] = [R.in_range(r, lo, hi) if r.shape[0] else np.zeros(0, bool) for r in self.rows]
        return self._masks[key]


def match_mask(rows, values):
    """bool[n]: the row's `width` bytes equal one of the list's values of exactly that length"""
    n, width = rows.shape
    keep = np.zeros(n, dtype=bool)
    for v in values:
        if len(v) == width:
            keep |= (rows == np.frombuffer(v, dtype=np.uint8)).all(axis=1)
    return keep


@functools.lru_cache(maxsize=None)
def string_case(width, layout):
    return StringCase(width, layout)


class IntCase:
    """An int32 column `ids` and an int8 column `tiny` over one layout (values -40 .. 40, 0 only where it is pinned), age / gate as
    StringCase's.  lists(form): [(values, what)] of the size that takes the form"""
    MEMBERS = [7, -13, 22, 39, -40]
    OUT = 99                                               # pinned "out": in no list

    def __init__(self, layout):
        self.layout = layout
        rng = np.random.default_rng(9000 + sum(LAYOUTS[layout]))
        self.ids = [np.zeros(n, np.int32) for n in LAYOUTS[layout]]
        pinned = {"sel": 7, "sel_dropped": 7, "out": self.OUT, "out_dropped": self.OUT, "zero": 0, "zero_dropped": 0}
        for si, r0, nv in tiles_of(layout):
            t = rng.integers(1, 41, size=nv) * rng.choice([-1, 1], size=nv)
            for r, what in pins(nv).items():
                t[r] = pinned[what]
            self.ids[si][r0:r0 + nv] = t
        self.tiny = [v.astype(np.int8) for v in self.ids]
        self.age, self.gate = zip(*int8_columns(rng, layout))

    def column(self, form):
        return self.tiny if form == "I8" else self.ids

    def lists(self, form, n_values):
        """the members, and fillers far from every row up to exactly n_values distinct values; with and without 0"""
        out = []
        for zero in (False, True):
            values = self.MEMBERS + ([0] if zero else [])
            fill = list(range(1000, 1000 + n_values - len(values))) if form != "I8" else list(range(50, 50 + max(0, n_values - len(values))))
            values = values + fill
            assert len(set(values)) == n_values and self.OUT not in values
            out.append((values, f"{n_values} values" + (", zero" if zero else "")))
        return out

    def masks(self, form, values):
        return [isin(c, values) for c in self.column(form)]


@functools.lru_cache(maxsize=None)
def int_case(layout):
    return IntCase(layout)


def expected_words(masks, layout):
    """per segment, the batch-major bitmap words of its mask"""
    return [R.bitmap_words(m, blocks_of(n)) for m, n in zip(masks, LAYOUTS[layout])]
