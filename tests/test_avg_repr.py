"""CPU suite: AvgDoubleAggr (ProjectAggregate.scala:60-75) -- its (sum, counter) state and repr(), which prints what the JVM prints
for (sum / counter).toString: java.math.BigDecimal.divide(counter, MathContext.DECIMAL128) of a sum with scale 1, then toString."""
from decimal import ROUND_HALF_EVEN, Context, Decimal

import pytest

from immutable3_amd import native
from immutable3_amd.operators import AvgDoubleAggr

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1

# (sum, counter, what BigDecimal prints): exact quotients keep the preferred scale 1 (or the few digits more they need), others
# round to 34 significant digits half-even; toString switches to E-notation below an adjusted exponent of -6
CASES = [
    (10, 4, "2.5"), (8, 4, "2.0"), (0, 5, "0.0"), (100, 3, "33.33333333333333333333333333333333"), (1, 10_000_000, "1E-7"),
    (-10, 4, "-2.5"), (-9, 3, "-3.0"), (2, 3, "0.6666666666666666666666666666666667"), (-2, 3, "-0.6666666666666666666666666666666667"),
    (1, 8, "0.125"), (1, 1_000_000, "0.000001"), (1, 3_000_000, "3.333333333333333333333333333333333E-7"), (-1, 20_000_000, "-5E-8"),
    (127 * 17_825_792, 17_825_792, "127.0"), (-128, 1, "-128.0"), (2 ** 31 - 1, 2, "1073741823.5"),
    (I64_MAX, 1, "9223372036854775807.0"), (I64_MIN, 1, "-9223372036854775808.0"), (I64_MIN, 2 ** 32, "-2147483648.0"),
    (I64_MAX, 7, "1317624576693539401.0"), (I64_MAX, 3, "3074457345618258602.333333333333333"),
    (I64_MIN, 3, "-3074457345618258602.666666666666667"), (I64_MAX, 2 ** 32, "2147483647.999999999767169356346130"),
]


def decimal128(s, n):
    return str(Context(prec=34, rounding=ROUND_HALF_EVEN).divide(Decimal(f"{s}.0"), Decimal(n)))


@pytest.mark.parametrize("s,n,text", CASES)
def test_repr_is_bigdecimal_divide_decimal128(s, n, text):
    a = AvgDoubleAggr("age", "age_avg")
    a.sum, a.counter = s, n
    assert a.repr() == text == decimal128(s, n)


def test_add_get_combine_follow_the_reference():
    a = AvgDoubleAggr("age", "age_avg")
    assert a.kind == native.AGG_SUM and a.get() == (0, 0)
    for v in (3, -1, 127.0, -128):
        a.add(v)
    assert a.get() == (1, 4) and a.repr() == "0.25"
    b = a.make()
    assert (b.col, b.alias, b.get()) == ("age", "age_avg", (0, 0))
    b.add(9)
    assert a.combine(b) is a and a.get() == (10, 5) and a.repr() == "2.0"
    with pytest.raises(ValueError):
        a.add(0.5)
    with pytest.raises(Exception):
        AvgDoubleAggr("age", "a").repr()      # 0 / 0: the reference's BigDecimal division throws too
