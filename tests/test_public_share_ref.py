"""tests/public_share_ref.py against the libsodium fixtures (no GPU, no library): the model of
dkg_public_shares reproduces public_share for every party from the round-3 commitments, the qualified and
reconstruct sets and the phase-5 disclosures alone, and S[0] is the master public key where nothing is
reconstructed.  This pins the yardstick of tests/test_gpu_public_shares.py."""
import pytest

from tests import public_share_ref as PR

FIXTURES = ["ceremony_n10_t4", "fault_recon_only_n10_t4", "fault_share_flip_n10_t4", "fault_a_generator_n10_t4",
            "fault_self_share_n10_t4", "fault_e_identity_n10_t4", "fault_recon_r2err_n16_t3", "ceremony_n2_t0",
            "ceremony_n3_t1", "ceremony_n11_t5", "ceremony_n16_t7", "ceremony_n8_t3_ck"]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_public_shares(golden, name):
    c = golden(name + ".json")
    n, t = c["n"], c["t"]
    A = bytes.fromhex(c["A"])
    V, st, wh, S = PR.public_shares(1, n, t, A, c["qualified"], list(range(n)), c["reconstruct"],
                                    PR.fixture_disclosures(c))
    assert st == [PR.OK] * n and wh == [-1] * n
    assert V == bytes.fromhex(c["public_share"])
    if not any(c["reconstruct"]):
        assert S[:32] == bytes.fromhex(c["mpk"])
    mask = [int(q and not r) for q, r in zip(c["qualified"], c["reconstruct"])]
    assert PR.commitment_sum(1, n, t, A, mask) == (S, [1])


def test_status_rule(golden):
    c = golden("fault_recon_only_n10_t4.json")
    n, q, r = c["n"], c["qualified"], c["reconstruct"]
    rec = [i for i in range(n) if r[i]]
    assert len(rec) == 2
    pairs = [(j + 1, i + 1) for i in rec for j in range(n)]
    assert PR.status(n, q, r, 3, pairs) == (PR.OK, -1)
    assert PR.status(n, q, r, 3, [p for p in pairs if p != (4, rec[1] + 1)]) == (PR.NO_DISCLOSURE, rec[1])
    assert PR.status(n, q, r, 3, []) == (PR.NO_DISCLOSURE, rec[0])
    used = [i for i in range(n) if q[i] and not r[i]]
    ap = [1] * n
    ap[used[2]] = ap[used[4]] = 0
    assert PR.status(n, q, r, 3, [], ap) == (PR.NO_COMMITMENT, used[2])  # the commitment comes first
    ap = [1] * n
    ap[rec[0]] = 0  # a reconstructed dealer's vector is not used
    assert PR.status(n, q, r, 3, pairs, ap) == (PR.OK, -1)
