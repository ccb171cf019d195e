"""dkg_ctx_phase_ms of the families that only the benchmark and the timing tools read: r24 / r2 / r4 (the
checks' pipeline), interp, full (one ceremony's hybrid kernels) and bfull (a batch's, summed over its chunks),
and a seats call after another family's marks were left uncollected.  Signs only: >= 0 where a phase is
recorded (> 0 where a kernel certainly ran), -1 where the call did not run or did not time it."""
import pytest

import dkg_amd
from tests.test_gpu import CK, H, dec_str
from tests.test_gpu_seats import Stack, seat_cols

pytestmark = pytest.mark.gpu

VERIFY = ("binomial", "stepping", "combine", "check")
ENC = ("enc_mul", "enc_encode", "enc_sym")
DEC = ("dec_decode", "dec_mul", "dec_encode", "dec_sym")
BENC = ("enc_decode", "enc_tab", "enc_e1", "enc_mul", "enc_encode", "enc_sym")


@pytest.fixture(scope="module")
def ctx():
    b = dkg_amd.Backend(0)
    yield b
    b.close()


@pytest.fixture()
def be(ctx):
    """The module's context on one stream, the setting under which phases are recorded."""
    try:
        ctx.set_streams(1)
        yield ctx
    finally:
        ctx.set_streams(2)


def shares(c):
    return H(c["E"]), H(c["A"]), H(c["s"]), H(c["s_prime"])


def test_fused_rounds(be, golden):
    c = golden("ceremony_n10_t4.json")
    n, t = c["n"], c["t"]
    be.env_init(t, n, CK)
    r = be.ceremony_verify(*shares(c), n, t)
    assert dec_str(r.dec2) == c["dec2"]
    ph = be.phase_times("r24")
    assert ph["binomial"] > 0 and ph["stepping"] > 0 and ph["check"] > 0 and ph["combine"] >= 0, ph


def test_rounds_in_protocol_order(be, golden):
    c = golden("ceremony_n3_t1.json")
    n, t = c["n"], c["t"]
    be.env_init(t, n, CK)
    try:
        be.set_overlap(False)
        be.ceremony_verify(*shares(c), n, t)
    finally:
        be.set_overlap(True)
    for tag in ("r2", "r4"):
        ph = be.phase_times(tag)
        assert all(ph[k] >= 0 for k in VERIFY), (tag, ph)


def test_interpolation(be, golden):
    c = golden("ceremony_n10_t4.json")
    n, t = c["n"], c["t"]
    be.env_init(t, n, CK)
    try:
        be.set_verify_mode(1)
        r = be.ceremony_verify(*shares(c), n, t)
    finally:
        be.set_verify_mode(0)
    assert dec_str(r.dec2) == c["dec2"]
    ph = be.phase_times("interp")
    assert all(ph[k] >= 0 for k in ("interpolate", "coef_check", "decide", "fallback")), ph


def test_full_mode(be, golden):
    import torch

    c = golden("full_n4_t1.json")
    n, t = c["n"], c["t"]
    be.env_init(t, n, CK)
    sk, pk = H(c["member_sk"]), H(c["member_pk"])
    dev = torch.device("cuda", 0)
    ta, tb, tr = (torch.tensor(list(H(c[k])), dtype=torch.uint8, device=dev) for k in ("a", "b", "enc_r"))
    r = be.ceremony_full_device(ta.data_ptr(), tb.data_ptr(), tr.data_ptr(), sk, pk, n, t)
    assert r.mpk.hex() == c["mpk"]
    ph = be.phase_times("full")
    assert all(ph[k] >= 0 for k in ENC + DEC), ph
    # the receivers' side alone: no encryption, so its phases of the run before are gone
    r = be.ceremony_verify_full(H(c["E"]), H(c["A"]), H(c["e1"]), H(c["ct"]), sk, n, t)
    assert r.mpk.hex() == c["mpk"]
    ph = be.phase_times("full")
    assert all(ph[k] == -1 for k in ENC) and all(ph[k] >= 0 for k in DEC), ph
    be.set_streams(2)  # chunk streams: nothing is timed, and the earlier records do not stay
    be.ceremony_verify_full(H(c["E"]), H(c["A"]), H(c["e1"]), H(c["ct"]), sk, n, t)
    ph = be.phase_times("full")
    assert all(ph[k] == -1 for k in ENC + DEC), ph


def test_batch_full_mode(be, golden):
    import torch

    c = golden("full_n4_t1.json")
    B, n, t = 3, c["n"], c["t"]
    master, c0 = H(c["master_seed"]), c["ceremony"]
    be.env_init(t, n, CK)

    def bfull():
        return {k: dkg_amd.lib().dkg_ctx_phase_ms(be.ctx, f"bfull.{k}".encode()) for k in BENC + DEC}

    dev = torch.device("cuda", 0)
    ta = torch.empty(32 * B * n * (t + 1), dtype=torch.uint8, device=dev)
    tb = torch.empty_like(ta)
    tr = torch.empty(64 * B * n * n, dtype=torch.uint8, device=dev)
    be.dealer_coefficients_device(master, c0, B, 0, n, t, ta.data_ptr(), tb.data_ptr())
    be.enc_randomness_device(master, c0, B, 0, n, n, t, tr.data_ptr())
    sk, pk = be.member_keys_batch(master, c0, B, n)
    assert sk[:32 * n].hex() == c["member_sk"]
    try:
        be.set_batch_full_chunk(1)  # three chunks, summed
        r = dkg_amd.ceremony_batch_full_device(be, B, n, t, ta.data_ptr(), tb.data_ptr(), tr.data_ptr(), sk, pk)
        assert r.mpk[0].hex() == c["mpk"]
        ph = bfull()
        assert all(v >= 0 for v in ph.values()), ph
        e1, ct = be.encrypt_shares_batch(pk, H(c["s"]) * B, H(c["s_prime"]) * B, H(c["enc_r"]) * B, B, n)
        assert e1[:64 * n * n].hex() == c["e1"]
        ph = bfull()
        assert all(ph[k] >= 0 for k in BENC) and all(ph[k] == -1 for k in DEC), ph
        s, _, _ = be.decrypt_shares_batch(sk, e1, ct, B, n)
        assert s == H(c["s"]) * B
        ph = bfull()
        assert all(ph[k] == -1 for k in BENC) and all(ph[k] >= 0 for k in DEC), ph
    finally:
        be.set_batch_full_chunk(0)


def test_seats_after_uncollected_marks(be, golden):
    """encrypt_shares on one stream marks full.* and collects nothing; the seats call after it records
    exactly what it records on a fresh context (test_gpu_seats.test_arguments_and_phases)."""
    f = golden("full_n4_t1.json")
    be.encrypt_shares(H(f["member_pk"]), H(f["s"]), H(f["s_prime"]), H(f["enc_r"]), f["n"], f["n"])
    c = golden("ceremony_n10_t4.json")
    st = Stack([c, c])
    n, t = st.n, st.t
    be.env_init(t, n, CK)
    sc, spc = seat_cols(st.s, n, [(1, 1)]), seat_cols(st.sp, n, [(1, 1)])
    assert dec_str(be.verify_seats(2, n, t, 2, [1], [1], st.E, sc, spc)) == st.expect(2, [(1, 1)])
    ph = be.phase_times("seats")
    assert ph["decrypt"] == -1 and ph["prove"] == -1
    assert ph["decode"] >= 0 and ph["eval"] > 0 and ph["check"] > 0
