"""Shapes of the tiled SASRec kernel tests (tests/test_sasrec_tiled_kernels_gpu.py; checked on the CPU by
tests/test_sasrec_tiled_cpu.py)  --  TEST INFRASTRUCTURE ONLY.

A table of (Case, tile, what): ``Case``, the inputs (every row drawn, the padding too) and the float64 reference are those of
tests/sasrec_cases.py; every figure comes from the kernels' own host-side queries (csrc/sasrec.hip), never from a literal.
Each case carries the first seed from 0 upward with which the float64 reference alone meets the conditions the comparisons
rest on (tests/test_sasrec_tiled_cpu.py holds that)."""
from collections import namedtuple

import sasrec_cases as K
from clsr_amd.ops import query
from sasrec_cases import Case

Tiled = namedtuple("Tiled", "case tile what")

BUDGET, C_MAX, NB_MAX, T_MAX, T_AT_40, T_AT_MAX = K.BUDGET, K.C_MAX, K.NB_MAX, K.T_MAX, K.T_AT_40, K.T_AT_MAX
TILE_MAX = 64


def default_tile(T, C):
    return query("clsr_sasrec_tiled_default_tile", T, C)


def lds_bytes(T, C, tile, training=1):
    return query("clsr_sasrec_tiled_lds_bytes", T, C, tile, training)


def lds_formula(T, C, tile, training=1):
    """k and v of the whole history, and one tile of t = min(tile, T) rows of everything else"""
    t = min(tile, T)
    return 4 * (2 * T * (C + 1) + t * (7 * (C + 1) + C // 2 + 1 if training else 3 * (C + 1)))


def t_longest(C):
    """Longest history the tiled kernels admit at width C with their default tile."""
    T = 0
    while T < T_MAX and default_tile(T + 1, C) > 0:
        T += 1
    return T


PARTS_CAP = query("clsr_sasrec_tiled_parts", 1 << 30, 4, 4, 8, 2)
T_LONG_MAX = t_longest(C_MAX)
NINE = Case(3, 9, 9, 4, 4, 1, 2, (9, 4, 6), 0, "T = 9, two heads (dh = 4)")

CASES = [
    Tiled(Case(2, 1, 1, 4, 4, 2, 1, (1,), 0, "T = 1"), 4, "T = 1 under a tile of 4"),
    Tiled(Case(5, 8, 8, 4, 4, 2, 1, (8, 4, 5, 0, 1), 0, "T = 8"), 4,
          "an exact multiple of the tile; lengths on a tile edge, one past it, 0 and 1"),
    Tiled(NINE, 4, "a ragged last tile"),
    Tiled(NINE, TILE_MAX, "one tile (tile >= T)"),
    Tiled(NINE, 1, "a tile of one row"),
    Tiled(Case(3, 9, 12, 4, 4, 1, 2, (1,), 0, "len = 1 inside T = 9; three rows of pos past T"), 4, "rows of pos past T"),
    Tiled(Case(2, 7, 7, 4, 4, NB_MAX, 1, (7, 3), 0, "the most blocks"), 4, "the most blocks"),
    Tiled(Case(2, 8, 8, C_MAX - 4, 4, 1, C_MAX // 4, (8, 5), 0, "the widest C with the most heads (dh = 4)"), 4,
          "the widest C with the most heads"),
    Tiled(Case(2, 8, 8, 4, C_MAX - 4, 2, 1, (7, 2), 0, "the widest C with one head, Dc > Di"), 4,
          "the widest C with one head, Dc > Di"),
    Tiled(Case(PARTS_CAP + 3, 4, 4, 4, 4, 2, 1, (2, 4, 1, 3, 4, 0, 1), 0, "the cap of the partial rows"), 2,
          "the persistent loop: three workgroups walk a second history"),
    Tiled(Case(2, T_AT_40 + 1, T_AT_40 + 1, 32, 8, 1, 1, (T_AT_40 + 1, 40), 0, "C = 40, one step past the resident limit"),
          default_tile(T_AT_40 + 1, 40), "the first shape the resident kernels refuse at C = 40"),
    Tiled(Case(2, 250, 250, 32, 8, 2, 1, (250, 131), 0, "the Kuaishou quick start's shape"), default_tile(250, 40),
          "T = 250 = Tmax at C = 40, two blocks"),
    Tiled(Case(1, T_MAX, T_MAX, 32, 8, 1, 2, (T_MAX,), 0, "the most steps at C = 40"), default_tile(T_MAX, 40),
          "T = %d at C = 40: %d of %d bytes" % (T_MAX, lds_bytes(T_MAX, 40, default_tile(T_MAX, 40)), BUDGET)),
]
if T_LONG_MAX > T_AT_MAX:
    CASES.append(Tiled(Case(2, T_LONG_MAX, T_LONG_MAX, 32, C_MAX - 32, 1, 2, (T_LONG_MAX, 11), 0,
                            "the longest history at C = %d" % C_MAX), default_tile(T_LONG_MAX, C_MAX),
                       "C = %d, T = %d under a tile of %d" % (C_MAX, T_LONG_MAX, default_tile(T_LONG_MAX, C_MAX))))
TILES_OF_NINE = [tc for tc in CASES if tc.case is NINE]
MIXED, MULTI, FIRST_PAST, KUAISHOU = CASES[1], CASES[9], CASES[10], CASES[11]
# refused by clsr_sasrec_supported, admitted by the tiled query
BOUNDARY = [FIRST_PAST] + ([CASES[-1]] if T_LONG_MAX > T_AT_MAX else [])

# (T, Tmax, C, blocks, heads, tile) and what is past
PAST = [((8, 8, 8, 1, 1, 0), "tile = 0"), ((8, 8, 8, 1, 1, TILE_MAX + 1), "tile = %d" % (TILE_MAX + 1)),
        ((T_MAX + 1, T_MAX + 1, 8, 1, 1, 4), "T past %d" % T_MAX)]
PAST += [((T, T, C_MAX, 1, 1, 1), "C = %d, T = %d: no tile fits" % (C_MAX, T)) for T in range(1, T_MAX + 1)
         if default_tile(T, C_MAX) == 0][:1]


def case_id(tc):
    return "%s-tile%d" % (K.case_id(tc.case), tc.tile)
