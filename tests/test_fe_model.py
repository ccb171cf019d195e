"""The limb-exact model of fe25519.h / sc25519.h (tests/fe_model.py) against plain big integers, on
the vectors the GPU tests feed the device (tests/test_gpu_field_ops.py, tests/test_gpu_scalar_ops.py):
every vector lies inside the range its primitive states, the classes that reach the edge of the
contract are present, and they -- not inputs of the suite's usual kind -- are what catches a wrong carry."""
import math

import pytest

from tests import fe_model as M

P, L = M.P, M.L


def _elements(op, out):
    return [out[10 * j:10 * j + 10] for j in range(len(out) // 10)]


def check_field(op, flavour, t, out, cls=""):
    """The checks of one field result, in the order that tells which side is wrong: the value, the
    output bound, the limb model, the representation of zero.  Shared with the GPU tests."""
    ref = M.fe_ref(op, t)
    where = (op, flavour, cls, t, out)
    if op in ("tobytes", "frombytes"):
        assert out == ref, where
        return
    for j, el in enumerate(_elements(op, out)):
        assert M.value(el) % P == ref[j], ("value", j) + where
        if op in M.TIGHT_OUT:
            assert M.is_tight(el), ("tight", j) + where
    assert out == M.fe_model(op, flavour, t), ("limb model",) + where
    if op in M.TIGHT_OUT and op != "abs":
        for j, el in enumerate(_elements(op, out)):
            if ref[j] == 0:
                assert el in (M.ZERO, M.P_LIMBS), ("zero representation", j) + where


def test_list_lengths():
    assert {k: len(v) for k, v in M.field_vectors().items()} == M.FIELD_COUNTS
    assert {k: len(v) for k, v in M.scalar_vectors().items()} == M.SCALAR_COUNTS


@pytest.mark.parametrize("op", sorted(M.FIELD_COUNTS))
def test_field_vectors_admissible(op):
    for cls, t in M.field_vectors()[op]:
        assert M.violations(op, t) == [], (op, cls, t)


def test_sq_uniform_bound_is_found_not_assumed():
    b = M.sq_uniform_max()
    assert not M.violations("sq", [b] * 10) and M.violations("sq", [b + 1] * 10)
    assert b >= int(2 ** 27.585)  # what the formulas hand fe_sq at most (fe25519.h)
    print("largest uniform fe_sq bound: 2^%.4f" % math.log2(b))


@pytest.mark.parametrize("flavour", [1, 2])
@pytest.mark.parametrize("op", sorted(set(M.FIELD_COUNTS) - {"invert", "pow22523"}))
def test_field_model_equals_reference(op, flavour):
    for cls, t in M.field_vectors()[op]:
        check_field(op, flavour, t, M.fe_model(op, flavour, t), cls)


@pytest.mark.parametrize("op", ["invert", "pow22523"])
def test_exponentiations_equal_reference(op):
    """Both flavours on the special values; the full list (a few hundred chains of 265 products per
    flavour) runs against the device, where the model is evaluated once per flavour."""
    for cls, t in M.field_vectors()[op]:
        if cls != "canon":
            for flavour in (1, 2):
                check_field(op, flavour, t, M.fe_model(op, flavour, t), cls)


def _traces(op):
    for cls, t in M.field_vectors()[op]:
        tr = {}
        if op == "mul":
            M.fe_mul(t[0:10], t[10:20], 1, trace=tr)
            M.fe_mul(t[0:10], t[10:20], 2, trace=tr)
        else:
            M.fe_sq(t[0:10], 1, trace=tr)
            M.fe_sq(t[0:10], 2, trace=tr)
        yield cls, tr


def test_hard_classes_present():
    for op in ("mul", "sq"):
        tr = list(_traces(op))
        canon = [t for c, t in tr if c == "canon"]
        fold = max(t["fold_carry"] for _, t in tr)
        # fe_sq's largest admissible input (the bisected uniform bound) carries 2^33.8 into the fold
        assert sum(t["fold_carry"] >= 1 << 32 for _, t in tr) >= 100 and fold >= 1 << (34 if op == "mul" else 33), (op, fold)
        assert max(t["col_max"] for _, t in tr) >= 1 << 63, op
        # inputs of the suite's usual kind stay far from that edge
        assert max(t["fold_carry"] for t in canon) < 1 << 30 and max(t["col_max"] for t in canon) < 1 << 60
        # the second carry out of h4 is no rarity (it takes what limb 3's column carried in); only its size grows
        assert any(t["h4_second"] for _, t in tr)
        assert any(t["h4_second"] >= 1 << 11 for _, t in tr) and all(t["h4_second"] < 1 << 10 for t in canon)


def _disagreements(op, flavour, mutant, classes=None):
    bad = set()
    for cls, t in M.field_vectors()[op]:
        if classes is None or cls in classes:
            out = M.fe_model(op, flavour, t, mutant)
            if [M.value(el) % P for el in _elements(op, out)] != M.fe_ref(op, t):
                bad.add(cls)
    return bad


@pytest.mark.parametrize("op", ["mul", "sq", "mul2", "sq2"])
def test_vectors_have_teeth(op):
    """FE_FOLD without its (h >> 32) term, and fe_carry64 with arithmetic shifts (columns from 2^63 up go
    negative), compute every random canonical-limb case right and are caught by the corner classes."""
    for flavour, mutant in ((1, "fold_hi"), (2, "signed")):
        assert _disagreements(op, flavour, mutant, {"canon"}) == set()
        caught = _disagreements(op, flavour, mutant)
        assert caught and "canon" not in caught, (op, mutant, caught)
        print(op, mutant, "caught by", sorted(caught))


@pytest.mark.parametrize("op", ["mul", "sq"])
def test_second_h4_carry_mutant(op):
    """fe_carry64 without the second carry out of h4 is wrong on the list -- and on random canonical limbs
    as well: h4 was cut to 26 bits before limb 3's carry (above 2^32 for any full-width input) came in,
    so that carry is nonzero on almost every input and the goldens already pin it.  What only the corner
    classes reach in fe_carry64 is the top bit of a column (test_vectors_have_teeth)."""
    caught = _disagreements(op, 2, "h4_second")
    assert caught and "canon" in caught and "corner" in caught, caught


# ------------------------------------------------------------------ scalars
@pytest.mark.parametrize("op", sorted(M.SCALAR_COUNTS))
def test_scalar_model_equals_reference(op):
    for _, t in M.scalar_vectors()[op]:
        M.sc_check(op, t, M.sc_model(op, t))


def test_scalar_vectors_in_range():
    v = M.scalar_vectors()
    assert all(M.val(t) < 2**277 for _, t in v["reduce9"])
    assert all(M.val(t[0:8]) < L and t[8] < 1 << 24 and M.val(t[9:17]) < L for _, t in v["mul_small_add"])
    assert all(M.val(t[0:8]) < L and t[8] < 1 << 11 and M.val(t[9:17]) < L and M.val(t[17:25]) < L
               for _, t in v["horner2"])
    assert all(M.val(t[0:10]) < 2**254 and t[10] <= 5 and t[11] < 1 << 13 and M.val(t[12:20]) < L for _, t in v["lazy"])
    for op in ("add", "sub", "mont_mul", "mul"):
        assert all(M.val(t[0:8]) < L and M.val(t[8:16]) < L for _, t in v[op])
    assert all(M.val(t) < L for _, t in v["neg"]) and all(0 < M.val(t) < L for _, t in v["mont_inv"])
    assert all(M.val(t) < 2**255 for _, t in v["radix16"])
    # both branches of sc_reduce9's final correction are taken
    taken = set()
    for _, t in v["reduce9"]:
        tr = {}
        M.sc_reduce9(t, tr)
        taken.add(tr["borrow"])
    assert taken == {False, True}
