"""The cost rule behind mode 0 of the sharded full-mode calls (dkg_key_comb_choice, a host function): which
comb of the recipient keys serves K = pk_q r -- 1 the radix-2^10 tables, 2 the signed radix-16 combs.  It
returns the kind with the smaller (cached ? 0 : build(keys)) + mul_per_item * keys * items_per_key; the
constants are exported (dkg_key_comb_constants) and every expectation below is computed from them."""
import math

import pytest

import dkg_amd
from dkg_amd.api import key_comb_constants

KEYS = [1, 2, 4, 10, 64, 130, 1024, 4096, 16384]


@pytest.fixture(scope="module")
def c():
    k = key_comb_constants()
    assert all(v > 0 for v in k.values()), k
    # the premise of having two kinds at all: radix 2^10 multiplies faster and builds slower
    assert k["mul10_ns_per_item"] < k["mul16_ns_per_item"]
    assert k["build10_us_per_key"] > k["build16_us_per_key"]
    return k


def _build_ns(c, kind, keys):
    return (c["build%s_floor_us" % kind] + c["build%s_us_per_key" % kind] * keys) * 1e3


def _cost_ns(c, kind, keys, items, cached):
    k = "10" if kind == 1 else "16"
    return (0 if cached else _build_ns(c, k, keys)) + c["mul%s_ns_per_item" % k] * keys * items


def _switch(c, keys):
    """items_per_key at which cold radix 2^10 stops being dearer than cold radix 16: the builds' gap over
    the per-key difference of the multiplications (0: radix 2^10 is never dearer, it wins at every count)."""
    gap = _build_ns(c, "10", keys) - _build_ns(c, "16", keys)
    if gap <= 0:
        return 0
    return gap / ((c["mul16_ns_per_item"] - c["mul10_ns_per_item"]) * keys)


def test_rule_is_the_smaller_cost(c):
    for keys in KEYS:
        for items in (1, 2, 8, 128, 256, 2048, 8192, 100_000, 10_000_000):
            for c10 in (0, 1):
                for c16 in (0, 1):
                    a, b = _cost_ns(c, 1, keys, items, c10), _cost_ns(c, 2, keys, items, c16)
                    if math.isclose(a, b, rel_tol=1e-9):
                        continue
                    assert dkg_amd.key_comb_choice(keys, items, c10, c16) == (2 if b < a else 1), (keys, items, c10, c16)


def test_a_cached_kind_wins_over_building_the_other(c):
    """Within a ceremony's range: a key serves at most 2 n items and n <= 16,384 here.  A cached radix-2^10
    set wins at EVERY count (it also multiplies faster).  A cached radix-16 set wins while its dearer
    multiplication stays under the other's build, items < build10 / (mul16 - mul10) per key -- asserted
    to lie beyond the range, so that inside it the cached kind always wins."""
    limit = c["build10_us_per_key"] * 1e3 / (c["mul16_ns_per_item"] - c["mul10_ns_per_item"])  # without the floor: less
    assert limit > 2 * 16384, limit
    for keys in KEYS:
        for items in (1, 2, 130, 256, 2048, 8192, 2 * 16384):
            assert dkg_amd.key_comb_choice(keys, items, True, False) == 1
            assert dkg_amd.key_comb_choice(keys, items, False, True) == 2
            assert dkg_amd.key_comb_choice(keys, items, True, True) == 1  # both held: the faster multiplication
    for keys in KEYS:
        assert dkg_amd.key_comb_choice(keys, 10**9, True, False) == 1


@pytest.mark.parametrize("keys", KEYS)
def test_cold_choice_is_monotone_with_one_switch(c, keys):
    """Nothing cached: radix 16 (cheap build) for few items per key, radix 2^10 from the switch point on,
    and the switch point is the one the constants give."""
    sw = _switch(c, keys)
    probe = sorted({1, 2, 3, 64, 256, 2048, 8192, 10**5, 10**6, 10**8} |
                   {max(1, int(sw) + d) for d in (-2, -1, 0, 1, 2, 3)})
    kinds = [dkg_amd.key_comb_choice(keys, i) for i in probe]
    switches = sum(1 for a, b in zip(kinds, kinds[1:]) if a != b)
    if sw == 0:
        assert kinds == [1] * len(probe)
    else:
        assert kinds[0] == 2 and kinds[-1] == 1 and switches == 1, list(zip(probe, kinds))
        first1 = probe[kinds.index(1)]
        assert abs(first1 - sw) <= 1.0 + 1e-6 * sw, (first1, sw)


def test_single_ceremony_sizes_start_cold_on_radix_16(c):
    """With the committed constants (profiles/shard_full_time.json: both the floor and the per-key cost of the
    radix-16 build are the smaller ones) a cold key set of any committee takes radix 16, and a cached
    radix-2^10 set is kept."""
    assert c["build16_floor_us"] < c["build10_floor_us"] and c["build16_us_per_key"] < c["build10_us_per_key"]
    for n in (1, 2, 4, 10, 64, 130, 1024, 4096):
        for shards in (1, 2, 3, 8):
            D = max(1, n // shards)
            assert dkg_amd.key_comb_choice(n, 2 * D) == 2, (n, D)
            assert dkg_amd.key_comb_choice(n, 2 * D, True, False) == 1
