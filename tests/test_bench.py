"""CPU checks of bench.py's accounting: the closed-form work and byte counts behind the roofline
fields, and the per-launch traffic read from the committed PMC passes (no GPU needed)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def test_algorithmic_bytes_binomial():
    # step r: position 0 copies C_k (load + store), positions 1..r load two points and store one
    n, t, U = 1024, 511, 2
    L = (t + 1) // U
    per_launch, launches = bench.algorithmic_bytes("binomial", n, t, U)
    assert launches == L - 1
    cols = 2 * n * U
    total = sum(cols * 160 * (2 + 3 * r) for r in range(1, L))
    assert per_launch * launches == pytest.approx(total)
    assert per_launch == pytest.approx(252968960.0)


def test_algorithmic_bytes_stepping_and_combine():
    n, t, U = 1024, 511, 2
    step, nl = bench.algorithmic_bytes("stepping", n, t, U)
    # the table once, D_0 out per receiver with its dense Z copy (40 B, for the affine addends)
    assert nl == 1 and step == 2 * n * U * (256 * 160 + n * (160 + 40))
    comb, nl = bench.algorithmic_bytes("combine", n, t, U)
    assert nl == 1 and comb == 2 * n * n * (2 * 128 + 160)  # two affine piece values in, P(j) out
    # scalars, the E and A columns, the decisions, and one 128-B comb entry per window of g and h
    w = bench.combw_windows()
    assert bench.algorithmic_bytes("check", n, t, U) == (n * n * (2 * 32 + 2 * 160 + 2 + 2 * w * 128), 1)


def test_pmc_traffic_matches_workload():
    """Every committed traffic file (profiles/pmc_traffic/, one per profiled workload) is found by its
    own key and by no other; the check-pipeline kernels' measured bytes are within 10 % of their
    algorithmic bytes (no re-reads) wherever the closed form covers the kernel."""
    import json
    names = sorted(x for x in os.listdir(bench.TRAFFIC_DIR) if x.endswith(".json"))  # superseded/ aside
    assert any(nm.endswith("_D.json") for nm in names), names  # the headline workload is profiled
    for nm in names:
        with open(os.path.join(bench.TRAFFIC_DIR, nm)) as f:
            doc = json.load(f)
        k = doc["key"]
        n, t, U, plen, B, mode = k["n"], k["t"], k["split"], k["split_len"], k["batch"], k["mode"]
        assert "FETCH_SIZE" in doc["source"] and "WRITE_SIZE" in doc["source"]
        for kern in ("binomial", "stepping", "combine"):
            got = bench.pmc_traffic(kern, n, t, U, plen, B, mode)
            if kern not in doc["kernels"]:
                assert got is None
                continue
            assert got is not None and got[0] == doc["kernels"][kern]["bytes_per_launch"], (nm, kern)
            per_wave = kern == "binomial" and doc["kernels"][kern]["fetch_launches"] <= 2 * B and B > 1
            alg, _ = bench.algorithmic_bytes(kern, n, t, U, plen, per_wave, B)
            if alg and not (kern == "stepping" and B > 1):  # the repacked tail phases: not in the closed form
                # the per-step binomial's model counts both operand reads of an item (3 x 160 B); the
                # second read of a position (items m and m+1 share e_m) may hit L2: down to 2/3 (n=4096)
                lo = 0.6 if kern == "binomial" and not per_wave else 0.9
                # the per-wave binomial (168 VGPRs, 3 waves per SIMD) also spills 36 B per lane to
                # scratch, outside the model: 1.12x in round 5
                hi = 1.15 if per_wave else 1.1
                assert lo < got[0] / alg < hi, (nm, kern, got[0] / alg)
        assert bench.pmc_traffic("binomial", n + 1, t, U, plen, B, mode) is None
        assert bench.pmc_traffic("binomial", n, t, U, plen, B, "other") is None


def test_closed_form_work_per_pair():
    """DESIGN.md section 2's per-pair figures at n=1024, t=511, U=2 (per pair per round), in VALU
    issue slots (the roofline's unit: half-rate instructions count 2) and in instructions."""
    n, t = 1024, 511
    pairs = n * n  # the closed form counts every (dealer, receiver) position
    w = bench.algorithmic_valu(n, t, 2, 2, ded=False)
    assert w["binomial"] / pairs == pytest.approx(1.036e6, rel=0.05)  # recoded multipliers (binom_digits)
    # stepping: 2 x 256 positions, the additions of position p stop after step n - 1 - p
    assert w["stepping"] / pairs == pytest.approx(1.094e6, rel=0.05)
    assert w["combine"] / pairs == pytest.approx(0.62e6, rel=0.05)
    wi = bench.algorithmic_valu(n, t, 2, 2, bench.INSTR, ded=False)
    assert wi["binomial"] / pairs == pytest.approx(0.59e6, rel=0.05)
    assert wi["stepping"] / pairs == pytest.approx(0.602e6, rel=0.05)
    assert wi["combine"] / pairs == pytest.approx(0.353e6, rel=0.05)
    for k in w:  # every primitive is mostly half-rate (v_mad_u64_u32) work
        assert 1.6 < w[k] / wi[k] < 2.0
    # the dedicated stepping additions (default) drop the product of the cached form
    wd = bench.algorithmic_valu(n, t, 2, 2)
    assert 0.88 < wd["stepping"] / w["stepping"] < 0.95
    # and the dedicated binomial items: two product-free cached forms, a zero test per addition
    assert 0.95 < wd["binomial"] / w["binomial"] < 0.98, wd["binomial"] / w["binomial"]
    # the fused schedule carries both rounds' tables through binomial, stepping and recombination
    f = bench.fused_valu(n, t, 2, ded=False)
    assert f["binomial"] == pytest.approx(2 * w["binomial"])


def test_short_combine_work():
    """Recombination with short lattice multipliers (k_combine_short): at U=3 one chain of ~169
    doublings over three NAFs replaces 253 doublings over the NAFs of y and y^2 (~17 % less work);
    at U=4 one chain of ~190 replaces two chains of 253.  The check pays one Montgomery product per
    scalar for b_j s."""
    import dkg_amd

    n, t = 64, 511
    for U, plen, lo, hi in ((3, 171, 0.78, 0.88), (4, 128, 0.58, 0.68)):
        mults = dkg_amd.split_multipliers(n, plen, U)
        short = bench.algorithmic_valu(n, t, 2, U, plen=plen, mults=mults, affine=False)
        powers = bench.algorithmic_valu(n, t, 2, U, plen=plen)
        assert lo < short["combine"] / powers["combine"] < hi, (U, short["combine"] / powers["combine"])
        # affine addends (default): mixed additions pay for the normalisation (k_affine_pieces)
        aff = bench.algorithmic_valu(n, t, 2, U, plen=plen, mults=mults)
        assert 0.95 < aff["combine"] / short["combine"] < 0.99, (U, aff["combine"] / short["combine"])
        assert short["check"] - powers["check"] == n * n * 2 * bench.VALU["sc_mont_mul"][1]
        assert short["binomial"] == powers["binomial"] and short["stepping"] == powers["stepping"]


def test_valu_table_matches_count_tool_format():
    """bench.VALU holds (instructions, issue slots) per primitive; slots between 1x and 2x."""
    for k, (ins, sl) in bench.VALU.items():
        assert ins <= sl <= 2 * ins, k


def test_split_pieces_and_bytes():
    """Uneven pieces (runtime.hip split_len): n=1100, t=549, U=2 with L=320 -> 320 + 230; the short
    last piece joins the binomial 90 steps late (fewer bytes and slots than two pieces of 320)."""
    assert bench.split_pieces(549, 2, 320) == ([320, 230], 320)
    assert bench.split_pieces(511, 3) == ([171, 171, 170], 171)
    assert bench.split_pieces(511, 2) == ([256, 256], 256)
    per, nl = bench.algorithmic_bytes("binomial", 1100, 549, 2, 320)
    assert nl == 319
    cols = 2 * 1100
    total = sum(cols * 160 * (2 + 3 * r) + cols * 160 * (2 + 3 * max(r - 90, 0)) for r in range(1, 320))
    assert per * nl == pytest.approx(total)
    w = bench.algorithmic_valu(1100, 549, 2, 2, plen=320)
    w_even = bench.algorithmic_valu(1100, 549, 2, 2)
    assert w["stepping"] == pytest.approx(w_even["stepping"], rel=0.01)  # the same 550 positions
    assert w_even["binomial"] < w["binomial"] < 1.1 * w_even["binomial"]


def test_hybrid_valu_closed_form():
    """Full mode's closed forms (bench.hybrid_valu): k_enc_mul prices 24 radix-2^11 windows of g plus 64
    radix-16 windows of pk_q per item; k_dec_mul_w4 the odd multiples, then an addition per nonzero
    width-4 window digit of sk_q and a doubling per digit below the top, for the 2n items of q."""
    n = 3
    sk = (5).to_bytes(32, "little") + (1).to_bytes(32, "little") + (2**252 + 3).to_bytes(32, "little")
    assert bench._wnaf(5, 4) == [5] and bench._wnaf(2**252 + 3, 4) == [3] + [0] * 251 + [1]
    assert bench._wnaf(23, 4) == [7, 0, 0, 0, 1]  # 23 = 16 + 7
    w = bench.hybrid_valu(n, sk)
    S = bench.SLOTS
    assert w["enc_mul"] == 2 * n * n * (bench.combw_windows() + bench.key_comb_windows()) * S["combw_window"]
    pre = S["ge_dbl_t"] + 3 * S["ge_add"] + 5 * S["ge_to_cached"]
    c5 = pre + S["ge_add_signed"]  # one digit: one addition onto the identity
    c1 = pre + S["ge_add_signed"]
    # the top digit's addition is followed by doublings: no T (ge_add_signed_not)
    cb = pre + S["ge_add_signed_not"] + S["ge_add_signed"] + 251 * S["ge_dbl_not"] + S["ge_dbl_t"]
    assert w["dec_mul"] == 2 * n * (c5 + c1 + cb)
    assert w["enc_sym"] == w["dec_sym"] == 2 * n * n * bench.HY_SYM_SLOTS


def test_cpu_baseline_small_batch():
    """The CPU baseline's sampler at config-5 scale: whole ceremonies in the sample, a positive rate."""
    r = bench.cpu_baseline(16, 7, 1.0, ceremonies=10)
    assert r["value"] > 0 and r["kind"] == "port" and "whole ceremonies" in r["sample"]
    assert r["batch_s_extrapolated"] == pytest.approx(10 * r["ceremony_s_extrapolated"])


def test_dump_outputs_arrays(tmp_path):
    """--dump-outputs: one float32 .npy per output field of the step's result (timings left out),
    bytes as their values, a list of 32-byte keys joined, an oversized array cut to the same
    seeded sample on every call."""
    import numpy as np

    from dkg_amd.api import BatchResult, CeremonyResult, Int32s

    r = CeremonyResult(n=3, t=1, mpk=bytes(range(32)), qualified=[1, 1, 0], r2_error=[0, 0, 0], r4_error=[0, 1, 0],
                       complaints2=[0, 2, 1], reconstruct=[0, 0, 1], n_qualified=2, phase4_error=0,
                       ms={"total": 1.5})
    bench.dump_outputs(str(tmp_path / "d"), r)
    got = {p.name[:-4]: np.load(p) for p in (tmp_path / "d").iterdir()}
    assert set(got) == {"n", "t", "mpk", "qualified", "r2_error", "r4_error", "complaints2", "reconstruct",
                        "n_qualified", "phase4_error"}  # no `ms`, no absent big outputs
    assert all(a.dtype == np.float32 and a.ndim == 1 for a in got.values())
    assert got["mpk"].tolist() == list(range(32)) and got["complaints2"].tolist() == [0, 2, 1]
    assert got["n_qualified"].tolist() == [2]
    big = bytes(i % 251 for i in range(bench.DUMP_MAX_ELEMS + 1000))
    b = BatchResult(B=2, n=1, t=0, mpk=[b"\x01" * 32, b"\x02" * 32], n_qualified=[1, 1], phase4_error=b"\0\0",
                    qualified=b"\1\1", r2_error=b"\0\0", r4_error=b"\0\0",
                    complaints2=Int32s((7).to_bytes(4, "little") * 2), reconstruct=b"\0\0", final_share=None,
                    public_share=None, dec2=big, dec4=None, ms={})
    a1, a2 = bench.result_arrays(b), bench.result_arrays(b)
    assert a1["mpk"].tolist() == [1.0] * 32 + [2.0] * 32 and a1["complaints2"].tolist() == [7.0, 7.0]
    assert "final_share" not in a1 and "dec4" not in a1
    assert a1["dec2"].size == bench.DUMP_MAX_ELEMS and np.array_equal(a1["dec2"], a2["dec2"])
    assert set(a1["dec2"].tolist()) <= set(range(251))
    assert sum(a.nbytes for a in a1.values()) <= 64e6


def test_ref_equiv_w2_matches_survey():
    """SURVEY.md 8(d)'s tabulated reference-equivalent work per verified share (dalek-3 cost model):
    W2 = A 8,647 (t=4); B 19,663; C 58,831; D 200,961; E 625,085 Fp-mults; W4 = D 198,549, E 622,673."""
    got = {t: bench.ref_equiv(2 * t + 1, t, 1.0) for t in (4, 31, 127, 511, 2047)}
    assert [got[t]["W2_fp_mults_per_share"] for t in (4, 31, 127, 511, 2047)] == [8647, 19663, 58831, 200961, 625085]
    assert got[511]["W4_fp_mults_per_share"] == 198549 and got[2047]["W4_fp_mults_per_share"] == 622673
    r = bench.ref_equiv(1024, 511, 12.5e6)
    assert r["ref_equiv_W2_fp_mults_per_s"] == pytest.approx(12.5e6 * 200961)


def test_binom_digits_cheapest_chain():
    """The binomial's multiplier recoding (points.h small_recode, bench.binom_digits: the NAF with a
    leading 1 0 -1 turned into 1 1) represents m and is the cheapest signed-binary double-and-add chain
    of every m < 256 under the build's slot costs, against every signed-digit representation up to
    one digit longer than the NAF."""
    import itertools

    V = bench.SLOTS

    def chain(ds):
        c = 0
        for i in range(len(ds) - 2, -1, -1):
            nz = ds[i] != 0
            c += V["ge_dbl_t"] if (nz or i == 0) else V["ge_dbl_not"]
            if nz:
                c += bench.add_cost(V, "ge_add_signed", i == 0) + V["fe_tight_zero"]
        return c

    saved = 0
    for m in range(1, 256):
        ds = bench.binom_digits(m)
        assert sum(d << i for i, d in enumerate(ds)) == m and ds[-1] == 1 and set(ds) <= {-1, 0, 1}
        naf = bench._naf(m)
        best = min(chain(list(r) + [1]) for L in range(1, len(naf) + 2)
                   for r in itertools.product((-1, 0, 1), repeat=L - 1)
                   if sum(d << i for i, d in enumerate(r)) + (1 << (L - 1)) == m)
        assert chain(ds) == best, m
        saved += chain(naf) - chain(ds)
    assert saved > 0
