"""The compiled scalar primitives of dkg_amd/csrc/sc25519.h at the edges of their stated input ranges
(dkg_sc_ops), against plain big integers mod l in canonical form: sc_reduce9 around every multiple of l
it can meet, at 2^277 - 1 and where the low part equals q delta (both branches of its correction), the
small-multiplier steps at their largest x with coefficients l - 1, the lazy accumulator from 2^254 - 1
through 0..5 steps of x = 8191, Montgomery products and the inversion on 0, 1, l - 1, R and R^2,
sc_reduce512 on all-ones and the wide-reduction KATs, the signed radix-16 recoding on nibble patterns
that carry through every digit.  The vectors are the lists tests/test_fe_model.py validates on the CPU."""
import pytest

import dkg_amd
from tests import fe_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.close()


@pytest.mark.parametrize("op", sorted(M.SCALAR_COUNTS))
def test_scalar_op(be, op):
    vec = M.scalar_vectors()[op]
    assert len(vec) == M.SCALAR_COUNTS[op]
    got = be.sc_ops(op, [t for _, t in vec])
    assert len(got) == M.SCALAR_COUNTS[op]
    for (_, t), out in zip(vec, got):
        M.sc_check(op, t, out)
        if op == "lazy":  # the folded accumulator word for word (its value is pinned only mod l)
            assert out == M.sc_model(op, t), (t, out)


def test_arguments(be):
    lib, ctx = dkg_amd._lib.lib(), be.ctx
    assert lib.dkg_sc_ops(ctx, 0, 0, None, None) == dkg_amd._lib.DKG_OK  # count == 0 touches nothing
    for op in (-1, len(be.SC_OPS)):
        assert lib.dkg_sc_ops(ctx, op, 0, None, None) == dkg_amd._lib.DKG_E_ARG
    with pytest.raises(dkg_amd.DkgError):  # more steps than SC_LAZY_STEPS
        be.sc_ops("lazy", [[0] * 10 + [6, 1] + [0] * 8])
    assert sorted(c for c, _, _ in be.SC_OPS.values()) == list(range(len(be.SC_OPS)))
