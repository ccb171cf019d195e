"""The compiled field primitives of dkg_amd/csrc/fe25519.h at the corners of their stated input ranges,
in both flavours of the products (dkg_fe_ops: 1 product scanning, 2 column sums), against plain big
integers and against the limb-exact model of tests/fe_model.py.

The vectors are the lists tests/test_fe_model.py validates on the CPU (every one admissible under
tools/fe_bounds.py): uniform limbs at the three stated corners of fe_mul and at fe_sq's largest
admissible bound, TIGHT maxima, checkerboards, the operands the group formulas build, representations
of 0 and p, and, for the pair products, one chain at a corner beside one on ordinary limbs.  They reach
what real points never do: a carry of 2^34 into FE_FOLD, column sums just below 2^64.  Per result, in
this order: the value mod p, the TIGHT output bound, the model's limbs word for word, and 0 in one of
the two forms fe_tight_zero knows.  Everything is exact."""
import pytest

import dkg_amd
from tests import fe_model as M
from tests.test_fe_model import check_field

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.close()


@pytest.mark.parametrize("flavour", [1, 2])
@pytest.mark.parametrize("op", sorted(M.FIELD_COUNTS))
def test_field_op(be, op, flavour):
    vec = M.field_vectors()[op]
    assert len(vec) == M.FIELD_COUNTS[op]
    got = be.fe_ops(flavour, op, [t for _, t in vec])
    assert len(got) == M.FIELD_COUNTS[op]
    for (cls, t), out in zip(vec, got):
        check_field(op, flavour, t, out, cls)


def test_arguments(be):
    lib, ctx = dkg_amd._lib.lib(), be.ctx
    assert lib.dkg_fe_ops(ctx, 1, 0, 0, None, None) == dkg_amd._lib.DKG_OK  # count == 0 touches nothing
    for flavour, op in ((0, 0), (3, 0), (1, -1), (1, len(be.FE_OPS))):
        assert lib.dkg_fe_ops(ctx, flavour, op, 0, None, None) == dkg_amd._lib.DKG_E_ARG
    assert sorted(c for c, _, _ in be.FE_OPS.values()) == list(range(len(be.FE_OPS)))
