"""The in-library multi-device context (dkg_multi_*, include/dkg_amd.h; dkg_amd/csrc/multi.cpp): one
process sharding a ceremony by dealer over several devices, one host thread per shard, exchanged by
peer copies into the first device.  On a one-GPU box the devices repeat ([0, 0], [0, 0, 0]): the
shards then share the GPU and the peer copies are device-local, which exercises every step of the
N-device path (ranges, padded gathers, combine, reconstruction on the owning shard, finalise).
Checked byte for byte against the libsodium goldens and the single-context run."""
import ctypes
import hashlib

import pytest

import dkg_amd
from dkg_amd import _lib
from dkg_amd._lib import DKG_E_ARG, DKG_OK
from tests.test_gpu import CEREMONIES, CK, FAULTS, H, _check_ceremony
from tests.test_gpu_batch_proven import faulted_ceremony
from tests.test_gpu_shard_proven import _fields, lists2, lists4, same_proven, single_full, single_plain, u32s

pytestmark = pytest.mark.gpu

SHARDS = [[0], [0, 0], [0, 0, 0]]


@pytest.fixture(scope="module", params=SHARDS, ids=lambda d: f"ws{len(d)}")
def mb(request):
    m = dkg_amd.MultiBackend(request.param)
    yield m
    m.close()


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.close()


@pytest.mark.parametrize("name", CEREMONIES + ["ceremony_n64_t31.json"])
def test_multi_honest_goldens(mb, golden, name):
    c = golden(name)
    n, t = c["n"], c["t"]
    if len(mb) > n:
        pytest.skip("more shards than dealers")
    mb.env_init(t, n, CK)
    a, b = dkg_amd.dealer_coefficients(H(c["master_seed"]), c["ceremony"], 0, n, t)
    r = mb.ceremony(a, b, n, t)
    assert r.E is None
    _check_ceremony(c, r, n)
    ms = mb.phase_ms()
    assert all(v >= 0 for v in ms.values()), ms
    assert r.ms["total"] > 0


@pytest.mark.parametrize("name", FAULTS)
def test_multi_fault_goldens(mb, golden, name):
    """Tampered broadcasts (committee.rs:1105-1313), including round-4 reconstruction on the owning
    shard and the disclosure-dependent mpk (fault_recon_*)."""
    c = golden(name)
    n, t = c["n"], c["t"]
    mb.env_init(t, n, CK)
    r = mb.ceremony_verify(H(c["E"]), H(c["A"]), H(c["s"]), H(c["s_prime"]), n, t)
    _check_ceremony(c, r, n)


def _digest(r):
    return {k: hashlib.sha256(getattr(r, k)).hexdigest() for k in ("dec2", "dec4", "final_share", "public_share")} | {
        "mpk": r.mpk.hex(), "qualified": r.qualified, "reconstruct": r.reconstruct, "r4_error": r.r4_error}


def test_multi_n1024_matches_single_context(be, golden):
    """BASELINE's headline size over two shards, from host coefficients and from per-shard device
    buffers, against one context's run of the same ceremony."""
    import torch

    n, t = 1024, 511
    a, b = dkg_amd.dealer_coefficients(bytes(range(32)), 7, 0, n, t)
    be.env_init(t, n, CK)
    want = _digest(be.ceremony(a, b, n, t))
    assert want["qualified"] == [1] * n
    m = dkg_amd.MultiBackend([0, 0])
    try:
        m.env_init(t, n, CK)
        assert _digest(m.ceremony(a, b, n, t)) == want
        N = t + 1
        bufs = []
        for i in range(2):
            d0, d1 = dkg_amd.shard_range(n, 2, i)
            bufs.append([torch.frombuffer(bytearray(x[32 * N * d0:32 * N * d1]), dtype=torch.uint8).to("cuda:0")
                         for x in (a, b)])
        r = m.ceremony_device([x[0].data_ptr() for x in bufs], [x[1].data_ptr() for x in bufs], n, t)
        assert _digest(r) == want
        ms = m.phase_ms()
        assert ms["shard_max"] >= ms["shard_min"] > 0
    finally:
        m.close()


# ---------------------------------------------------------------- the eight ceremony entry points, one driver
# name -> (entry point, the arguments between t and `out`, the arguments after `out`, the required pointers)
EIGHT = {
    "run": ("dkg_multi_ceremony_run", ["a", "b"], [], ["a", "b"]),
    "run_device": ("dkg_multi_ceremony_run_device", ["pa", "pb"], [], ["pa", "pb"]),
    "verify": ("dkg_multi_ceremony_verify", ["E", "A", "s", "sp"], [], ["E", "A", "s", "sp"]),
    "run_full": ("dkg_multi_ceremony_run_full", ["a", "b", "r", "gsk", "gpk"], [], ["a", "b", "r", "gsk", "gpk"]),
    "run_full_device": ("dkg_multi_ceremony_run_full_device", ["pa", "pb", "pr", "gsk", "gpk"], [],
                        ["pa", "pb", "pr", "gsk", "gpk"]),
    "verify_full": ("dkg_multi_ceremony_verify_full", ["E", "A", "e1", "ct", "sk"], [], ["E", "A", "e1", "ct", "sk"]),
    "verify_proven": ("dkg_multi_ceremony_verify_proven",
                      ["E", "A", "s", "sp", "f1", "f3", "C4", "acc4", "acd4", "sh4", "rn4"], ["v4", "st", "ri"],
                      ["E", "A", "s", "sp"]),
    "verify_full_proven": ("dkg_multi_ceremony_verify_full_proven",
                           ["E", "A", "e1", "ct", "sk", "pk", "C", "acc", "acd", "proofs", "f3", "C4", "acc4", "acd4",
                            "sh4", "rn4"], ["v2", "dis", "v4", "st", "ri"], ["E", "A", "e1", "ct", "sk", "pk"]),
}


class Eight:
    """The faulted n = 10, t = 4 ceremony (received broadcasts, complaint lists) and full_n10_t4.json (the
    generate modes) as the eight entry points take them over three shards, and the single-context calls'
    results on the same inputs."""

    def __init__(self, be, golden):
        import torch

        cer = faulted_ceremony(golden)
        cer["s"], cer["s_prime"] = cer.pop("shares")
        g = golden("full_n10_t4.json")
        self.n, self.t, self.cer = cer["n"], cer["t"], cer
        n, t, N = self.n, self.t, self.t + 1
        a, b = dkg_amd.dealer_coefficients(H(g["master_seed"]), g["ceremony"], 0, n, t)
        r, gsk, gpk = H(g["enc_r"]), H(g["member_sk"]), H(g["member_pk"])
        self.keep = [[torch.frombuffer(bytearray(x[w * d0:w * d1]), dtype=torch.uint8).to("cuda:0")
                      for d0, d1 in (dkg_amd.shard_range(n, 3, i) for i in range(3))]
                     for x, w in ((a, 32 * N), (b, 32 * N), (r, 64 * n))]
        self.ptrs = [[x.data_ptr() for x in row] for row in self.keep]
        a2, d2, pr = lists2(cer["c2"])
        a4, d4, s4, r4 = lists4(cer["c4"])
        self.lists2, self.lists4 = (a2, d2, pr), (a4, d4, s4, r4)
        self.args = dict(a=a, b=b, r=r, gsk=gsk, gpk=gpk, E=cer["E"], A=cer["A"], s=cer["s"], sp=cer["s_prime"],
                         e1=cer["e1"], ct=cer["ct"], sk=cer["sk"], pk=cer["pk"], f1=None, f3=None, C=len(a2),
                         acc=u32s(a2), acd=u32s(d2), proofs=pr, C4=len(a4), acc4=u32s(a4), acd4=u32s(d4), sh4=s4, rn4=r4)
        be.env_init(t, n, CK)
        full = be.ceremony_verify_full(H(g["E"]), H(g["A"]), H(g["e1"]), H(g["ct"]), gsk, n, t)
        plain = be.ceremony(a, b, n, t)
        self.want = {"run": plain, "run_device": plain, "run_full": full, "run_full_device": full,
                     "verify": be.ceremony_verify(cer["E"], cer["A"], cer["s"], cer["s_prime"], n, t),
                     "verify_full": be.ceremony_verify_full(cer["E"], cer["A"], cer["e1"], cer["ct"], cer["sk"], n, t),
                     "verify_proven": single_plain(be, cer, cer["c4"]),
                     "verify_full_proven": single_full(be, cer, cer["c2"], cer["c4"])}

    def call(self, m, name):
        x, n, t = self.args, self.n, self.t
        pa, pb, pr = self.ptrs
        return {"run": lambda: m.ceremony(x["a"], x["b"], n, t),
                "run_device": lambda: m.ceremony_device(pa, pb, n, t),
                "verify": lambda: m.ceremony_verify(x["E"], x["A"], x["s"], x["sp"], n, t),
                "run_full": lambda: m.ceremony_full(x["a"], x["b"], x["r"], x["gsk"], x["gpk"], n, t),
                "run_full_device": lambda: m.ceremony_full_device(pa, pb, pr, x["gsk"], x["gpk"], n, t),
                "verify_full": lambda: m.ceremony_verify_full(x["E"], x["A"], x["e1"], x["ct"], x["sk"], n, t),
                "verify_proven": lambda: m.ceremony_verify_proven(x["E"], x["A"], x["s"], x["sp"], None, None,
                                                                  *self.lists4, n, t),
                "verify_full_proven": lambda: m.ceremony_verify_full_proven(
                    x["E"], x["A"], x["e1"], x["ct"], x["sk"], x["pk"], *self.lists2, *self.lists4, n, t)}[name]()

    def raw(self, m, name, null=None, shares_out=False):
        """The entry point through the C ABI with argument `null` passed as NULL, or with a non-null out->s."""
        fn, before, after, _ = EIGHT[name]
        i32 = ctypes.c_int32
        args = dict(self.args, st=ctypes.byref(i32()), ri=ctypes.byref(i32()), v2=(i32 * 16)(), v4=(i32 * 16)(),
                    dis=(i32 * self.n)(), **{k: (ctypes.c_void_p * 3)(*p) for k, p in zip(("pa", "pb", "pr"), self.ptrs)})
        if null is not None:
            args[null] = None
        o, bufs = m._out(self.n, self.t)
        keep = ctypes.create_string_buffer(32 * self.n * self.n)
        if shares_out:
            o.s = ctypes.cast(keep, ctypes.c_void_p)
        return getattr(_lib.lib(), fn)(m._m, self.n, self.t, *(args[k] for k in before), ctypes.byref(o),
                                       *(args[k] for k in after))


@pytest.fixture(scope="module")
def eight(be, golden):
    return Eight(be, golden)


def _same(name, got, want):
    if "proven" in name:
        same_proven(got, want, "full" in name)
    else:
        assert _fields(got) == _fields(want), name


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_eight_entry_points_share_one_context(eight, order):
    """The eight entry points one after another on one MultiBackend([0, 0, 0]) (dealers 3, 3, 4), in one
    order and in the reverse one: each result equals the single-context call's on the same inputs."""
    m = dkg_amd.MultiBackend([0, 0, 0])
    try:
        m.env_init(eight.t, eight.n, CK)
        names = list(EIGHT) if order == "forward" else list(EIGHT)[::-1]
        for name in names + names[:2]:
            _same(name, eight.call(m, name), eight.want[name])
    finally:
        m.close()


def test_eight_entry_points_argument_rule(eight):
    """Each of the eight rejects every required pointer passed NULL with DKG_E_ARG and a message of its own
    in dkg_multi_last_error (not the one an earlier failure left), rejects a non-null out->s, and the context
    serves the call afterwards."""
    lib = _lib.lib()
    m = dkg_amd.MultiBackend([0, 0, 0])
    try:
        m.env_init(eight.t, eight.n, CK)
        for name, (_, _, _, required) in EIGHT.items():
            for null in required:
                o, _bufs = m._out(eight.n, eight.t)
                assert lib.dkg_multi_ceremony_run(m._m, eight.n, eight.n, eight.args["a"], eight.args["b"],
                                                  ctypes.byref(o)) == DKG_E_ARG  # t too large: another message
                stale = lib.dkg_multi_last_error(m._m)
                assert eight.raw(m, name, null) == DKG_E_ARG, (name, null)
                msg = lib.dkg_multi_last_error(m._m)
                assert msg and msg != stale, (name, null)
            assert eight.raw(m, name, shares_out=True) == DKG_E_ARG, name
            assert eight.raw(m, name) == DKG_OK, name
            _same(name, eight.call(m, name), eight.want[name])
    finally:
        m.close()


def test_multi_rejects_bad_arguments(golden):
    with pytest.raises(dkg_amd.DkgError):
        dkg_amd.MultiBackend([])
    with pytest.raises(dkg_amd.DkgError):
        dkg_amd.MultiBackend([0, 99])
    m = dkg_amd.MultiBackend([0, 0, 0])
    try:
        m.env_init(0, 2, CK)
        a, b = dkg_amd.dealer_coefficients(bytes(32), 0, 0, 2, 0)
        with pytest.raises(dkg_amd.DkgError):
            m.ceremony(a, b, 2, 0)  # three shards, two dealers
        with pytest.raises(dkg_amd.DkgError):
            m.ceremony(a, b, 2, 1)  # committee.rs:73
    finally:
        m.close()
